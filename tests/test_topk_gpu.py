"""lgc_mask_topk (k_mask_topk, csrc/lgconv_serve.hip) on every path it takes, against the stable-sort reference of
tests/topk_support.py: the indices must EQUAL the reference's -- (value descending, index ascending), NaN first -- and
out_value must hold the reference's values bit for bit (any NaN matches any NaN).  tests/test_topk_host.py proves on the
CPU that the case table reaches the short cut, the register radix passes and the streaming passes, each with and
without a tie cut carried across 1,024-column slices; nothing here branches on the route."""
import numpy as np
import pytest
import torch

import topk_support as ts

from gnn_ecommerce_amd import _native, propagate

pytestmark = pytest.mark.gpu

E_INVAL, E_RANGE = -1, -4          # LGC_E_INVAL, LGC_E_RANGE (include/lgconv_hip.h)


def to_dev(a, device):
    """A device tensor with the numpy array's values AND row stride (a column slice stays a column slice)."""
    if a is None:
        return None
    base = a.base if a.base is not None and a.ndim == 2 and a.strides[0] != a.shape[1] * a.itemsize else None
    if base is None:
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)
    offset = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    assert base.ndim == 2 and base.flags.c_contiguous and 0 <= offset and offset + a.shape[1] <= base.shape[1]
    return torch.from_numpy(base).to(device)[:, offset:offset + a.shape[1]]


def call(scores, seen, lists, k, with_value=True):
    """lgc_mask_topk through the C ABI: (return code, indices [rows, k], values [rows, k])."""
    rows, cols = scores.shape
    idx = torch.full((rows, k), -7, dtype=torch.int64, device=scores.device)
    val = torch.full((rows, k), -7.0, dtype=torch.float32, device=scores.device) if with_value else None
    lib = _native.load()
    with torch.cuda.device(scores.device):
        code = lib.lgc_mask_topk(_native.ptr(scores), scores.stride(0), _native.ptr(seen), 0 if seen is None else seen.stride(0),
                                 _native.ptr(lists.ptr) if lists else None, _native.ptr(lists.items) if lists else None,
                                 _native.ptr(lists.users) if lists else None, rows, cols, k, _native.ptr(idx), _native.ptr(val),
                                 _native.stream_of(scores.device))
    return code, idx, val


def seen_lists(lists, device):
    if lists is None:
        return None
    return propagate.SeenLists(to_dev(lists.ptr, device), to_dev(lists.items, device), to_dev(lists.rows, device))


def first_difference(got, want):
    bad = np.argwhere(got != want)
    r, c = bad[0]
    return f"{len(bad)} entries differ, first at row {r} rank {c}: got {got[r, c]}, want {want[r, c]}"


@pytest.mark.parametrize("name", ts.CASE_NAMES)
def test_mask_topk_equals_the_stable_sort_reference(device, name):
    c = ts.case(name)
    scores = to_dev(c.scores, device)
    assert scores.stride(0) == c.scores.strides[0] // 4
    for form, dense, lists in c.forms:
        seen, lst = to_dev(dense, device), seen_lists(lists, device)
        assert seen is None or seen.stride(0) == dense.strides[0] // 4
        want_idx, want_val = ts.topk_ref(c.masked(form), max(c.ks))            # one order: a smaller k is its prefix
        for k in c.ks:
            where = f"{name} / {form} / k={k}"
            code, idx, val = call(scores, seen, lst, k)
            assert code == 0, where
            got_idx, got_val = idx.cpu().numpy(), val.cpu().numpy()
            assert np.array_equal(got_idx, want_idx[:, :k]), f"{where}: {first_difference(got_idx, want_idx[:, :k])}"
            assert ts.values_match(got_val, want_val[:, :k]), where
            code2, idx2, val2 = call(scores, seen, lst, k)                     # once more: the same bits
            assert code2 == 0 and torch.equal(idx2, idx) and torch.equal(val2.view(torch.int32), val.view(torch.int32)), where
            code3, idx3, _ = call(scores, seen, lst, k, with_value=False)      # out_value is optional
            assert code3 == 0 and torch.equal(idx3, idx), where
            assert torch.equal(propagate.mask_topk(scores, lst if lst is not None else seen, k), idx), where


def test_list_mask_limit_and_argument_errors(device):
    """The list form holds one bit per column in 120 KiB of LDS: 983,040 columns pass, one more is LGC_E_RANGE -- while the
    dense mask and no mask take the wider row (the case past_list_limit).  Arguments that make no sense are LGC_E_INVAL, and
    neither return touches the outputs."""
    cols = ts.LIST_COLS_MAX + 1
    scores = torch.zeros((1, cols), dtype=torch.float32, device=device)
    lists = propagate.SeenLists(torch.zeros(2, dtype=torch.int64, device=device), torch.zeros(1, dtype=torch.int64, device=device), None)
    code, idx, val = call(scores, None, lists, 20)
    assert code == E_RANGE and bool((idx == -7).all()) and bool((val == -7.0).all())
    with pytest.raises(_native.NativeLibraryError):
        propagate.mask_topk(scores, lists, 20)
    assert call(scores[:, :ts.LIST_COLS_MAX], None, lists, 20)[0] == 0           # a view one column narrower: accepted
    assert call(scores, None, None, 20)[0] == 0 and call(scores, scores, None, 20)[0] == 0
    assert call(scores, None, None, ts.K_MAX + 1)[0] == E_RANGE

    small = torch.zeros((2, 40), dtype=torch.float32, device=device)
    lib = _native.load()
    out = torch.full((2, 8), -7, dtype=torch.int64, device=device)
    stream = _native.stream_of(device)
    p = _native.ptr

    def raw(scores_p=p(small), s_stride=40, seen_p=None, m_stride=0, ptr_p=None, items_p=None, n_rows=2, n_cols=40, k=8, out_p=p(out)):
        with torch.cuda.device(device):
            return lib.lgc_mask_topk(scores_p, s_stride, seen_p, m_stride, ptr_p, items_p, None, n_rows, n_cols, k, out_p, None, stream)

    assert raw() == 0
    out.fill_(-7)
    assert raw(k=0) == E_INVAL and raw(k=41) == E_INVAL                          # k outside [1, n_cols]
    assert raw(n_cols=0) == E_INVAL and raw(n_rows=-1) == E_INVAL
    assert raw(s_stride=39) == E_INVAL                                           # rows would overlap
    assert raw(seen_p=p(small), m_stride=39) == E_INVAL
    assert raw(scores_p=None) == E_INVAL and raw(out_p=None) == E_INVAL
    assert raw(seen_p=p(small), m_stride=40, ptr_p=p(lists.ptr), items_p=p(lists.items)) == E_INVAL      # both mask forms
    assert raw(ptr_p=p(lists.ptr)) == E_INVAL                                    # lists without items
    assert raw(n_rows=0) == 0                                                    # nothing to do is not an error
    torch.cuda.synchronize(device)
    assert bool((out == -7).all())
