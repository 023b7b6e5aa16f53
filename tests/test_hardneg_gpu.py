"""lgc_sample_hard_triples on the device, through the C ABI, against tests/hardneg_support.py: the reference walks the
sampler's stream in Python integers and takes its scores from lgc_score_rows' panel of the same two tables, so negatives,
attempts, counts, positives and the status word must be equal and the winner's score bit-equal (any NaN for any NaN).  The
cases -- widths around the 16-byte groups, padded and misaligned tables with NaN in every float that must not be read,
candidate counts around the rounds of 64 attempts, ignore sets built so that the walk ends at attempts 64, 65, ..., ties and
special values -- come from the reference alone (tests/test_hardneg_host.py checks that they do what their names say)."""
import numpy as np
import pytest
import torch

import hardneg_support as hs
import sampler_support as ss
import topk_support as ts
from tests_support import sampler_lists

import gnn_ecommerce_amd as lg
from gnn_ecommerce_amd import _native, synth
from gnn_ecommerce_amd.sampler import TripleSampler

pytestmark = pytest.mark.gpu


class World:
    """A case on the device: CSRs, the two poisoned table buffers, lgc_score_rows' panel and the reference's records."""

    def __init__(self, device, c):
        self.b = b = hs.build(c)
        self.c, self.device = c, device
        dev = lambda a, dt: torch.tensor(list(a) or [0], dtype=dt, device=device)
        (pp, pi), (ip, ii) = b.csrs
        self.csr = [dev(pp, torch.int32), dev(pi, torch.int64), dev(ip, torch.int32), dev(ii, torch.int64)]
        self.users = dev(b.users, torch.int64)
        self.user_buf = torch.from_numpy(hs.poisoned(b.user_table, b.user_stride, c.uoff)).to(device)
        self.item_buf = torch.from_numpy(hs.poisoned(b.item_table, b.item_stride, c.ioff)).to(device)
        self.user_ptr = self.user_buf.data_ptr() + 4 * c.uoff
        self.item_ptr = self.item_buf.data_ptr() + 4 * c.ioff
        assert self.user_buf.data_ptr() % 16 == 0 and self.item_buf.data_ptr() % 16 == 0
        panel = torch.full((b.n_users, b.n_items), -7.0, device=device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            code = _native.load().lgc_score_rows(self.user_ptr, b.user_stride, b.n_users, None, b.n_users, self.item_ptr,
                                                 b.item_stride, b.n_items, c.dim, panel.data_ptr(), b.n_items,
                                                 status.data_ptr(), _native.stream_of(device))
        assert code == 0 and int(status.item()) == 0
        self.panel = panel.cpu().numpy()
        self.score = lambda u, item: self.panel[u, item]

    def reference(self, n_cand=None):
        c, b = self.c, self.b
        recs = hs.walk(b.users, b.csrs, b.n_users, b.n_items, c.seed, c.step, n_cand or c.n_cand, self.score)
        score = np.array([0.0 if r.bad else self.panel[r.user, r.neg - b.n_users] for r in recs], dtype=np.float32)
        status = 0
        for r in recs:
            status |= r.status
        return recs, score, status

    def launch(self, n_cand=None, optional=True):
        """One launch: dict of numpy outputs; every output has a guard element before and behind it."""
        c, b, n = self.c, self.b, self.c.n
        kinds = dict(pos=torch.int64, neg=torch.int64, score=torch.float32, attempt=torch.int32, admissible=torch.int32)
        out = {k: torch.full((n + 2,), -9, dtype=dt, device=self.device) for k, dt in kinds.items()}
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        at = lambda k: out[k][1:].data_ptr()
        opt = [at("score"), at("attempt"), at("admissible")] if optional else [None, None, None]
        with torch.cuda.device(self.device):
            code = _native.load().lgc_sample_hard_triples(
                self.users.data_ptr(), n, *(t.data_ptr() for t in self.csr), b.n_users, b.n_items, c.seed, c.step,
                n_cand or c.n_cand, self.user_ptr, b.user_stride, self.item_ptr, b.item_stride, c.dim, at("pos"), at("neg"),
                *opt, status.data_ptr(), _native.stream_of(self.device))
        assert code == 0
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for k, v in got.items():
            assert v[0] == -9 and v[-1] == -9, f"{k}: written outside [0, n)"
            got[k] = v[1:-1]
        got["status"] = int(status.item())
        return got


def agree(w, n_cand=None):
    recs, score, status = w.reference(n_cand)
    got = w.launch(n_cand)
    for name, want in (("pos", [r.pos for r in recs]), ("neg", [r.neg for r in recs]), ("attempt", [r.attempt for r in recs]),
                       ("admissible", [r.admissible for r in recs])):
        bad = np.flatnonzero(got[name] != np.array(want, dtype=np.int64))
        assert bad.size == 0, f"{w.c.name} {name}: {bad.size} of {w.c.n} differ, first at sample {bad[0]} (user " \
                              f"{recs[bad[0]].user}): got {got[name][bad[0]]}, want {want[bad[0]]}"
    assert got["status"] == status, f"{w.c.name}: status {got['status']}, want {status}"
    same = np.isnan(got["score"]) & np.isnan(score) | (ts.bits_of(got["score"]) == ts.bits_of(score))
    assert ts.values_match(got["score"], score), f"{w.c.name} neg_score: sample {np.flatnonzero(~same)[0]} differs"
    return recs, got


_worlds = {}


def world(device, name):
    """The device copy of a case, built once and left unchanged."""
    if name not in _worlds:
        _worlds[name] = World(device, hs.CASES[hs.CASE_NAMES.index(name)])
    return _worlds[name]


@pytest.mark.parametrize("name", hs.CASE_NAMES)
def test_case_matches_the_reference(device, name):
    w = world(device, name)
    recs, got = agree(w)
    for i, role in w.b.expect.items():                       # what the case was built for did happen on the device
        want = w.c.n_cand if role != "short" else recs[i].admissible
        assert got["admissible"][i] == want
    if w.c.kind == "zero":                                   # a table of zeros: the uniform sampler at any n_cand
        b = w.b
        pos, neg, status = ss.sample_ref(b.users, *b.csrs[0], *b.csrs[1], b.n_users, b.n_items, w.c.seed, w.c.step)
        assert got["pos"].tolist() == pos and got["neg"].tolist() == neg and got["status"] == status
        assert not got["score"].any() and not np.signbit(got["score"]).any()


@pytest.mark.parametrize("name", ["dim64", "dim90_pad3", "specials", "at64_m2"])
@pytest.mark.parametrize("n_cand", [1, 2, 63, 64, 65, 128, 255, 256])
def test_candidate_counts_on_one_world(device, name, n_cand):
    agree(world(device, name), n_cand)


@pytest.mark.parametrize("name", ["dim64", "m1", "dim90", "specials", "one_item", "step_top", "short", "dim64_both_bases_off"])
def test_one_candidate_is_lgc_sample_triples_bit_for_bit(device, name):
    w = world(device, name)
    c, b = w.c, w.b
    pos = torch.full((c.n,), -9, dtype=torch.int64, device=device)
    neg = torch.full((c.n,), -9, dtype=torch.int64, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        code = _native.load().lgc_sample_triples(w.users.data_ptr(), c.n, *(t.data_ptr() for t in w.csr), b.n_users, b.n_items,
                                                 c.seed, c.step, pos.data_ptr(), neg.data_ptr(), status.data_ptr(),
                                                 _native.stream_of(device))
    assert code == 0
    got = w.launch(1)
    assert np.array_equal(got["pos"], pos.cpu().numpy()) and np.array_equal(got["neg"], neg.cpu().numpy())
    assert got["status"] == int(status.item())
    assert set(got["admissible"].tolist()) <= {0, 1}


@pytest.mark.parametrize("name", ["dim64", "specials_m256", "duplicate_rows_d90", "dim5"])
def test_two_runs_give_the_same_bytes_and_null_outputs_change_nothing(device, name):
    w = world(device, name)
    first, second, bare = w.launch(), w.launch(), w.launch(optional=False)
    for k in ("pos", "neg", "score", "attempt", "admissible"):
        assert first[k].tobytes() == second[k].tobytes(), k
    assert first["status"] == second["status"] == bare["status"]
    assert np.array_equal(first["pos"], bare["pos"]) and np.array_equal(first["neg"], bare["neg"])
    for k in ("attempt", "admissible"):                      # the guards' value: nothing was written
        assert (bare[k] == -9).all(), k
    assert (bare["score"] == -9.0).all()


# ----------------------------------------------------------------------------------------
# the Python layer
# ----------------------------------------------------------------------------------------
def test_sample_hard_with_one_candidate_is_sample(device):
    n_users, n_items, seed = 60, 25, 3
    order, pos, ign = sampler_lists(n_users, n_items, 0)
    plain = TripleSampler(n_users, n_items, pos, ign, device, seed=seed)
    hard = TripleSampler(n_users, n_items, pos, ign, device, seed=seed)
    zeros = TripleSampler(n_users, n_items, pos, ign, device, seed=seed)
    table = torch.randn(n_users + n_items, 24, device=device, generator=torch.Generator(device=device).manual_seed(1))
    wide = torch.zeros(n_users + n_items, 31, device=device)
    for t in range(3):
        want = plain.sample(32)
        got = hard.sample_hard(32, table[:, :20] if t == 1 else table, candidates=1)      # a view with a longer row stride
        flat = zeros.sample_hard(32, wide[:, :24], candidates=64)
        assert len(got) == 3 and hard.step == plain.step == zeros.step == t + 1
        for a, b, c in zip(want, got, flat):
            assert torch.equal(a, b) and torch.equal(a, c) and b.dtype == torch.int64
    assert int(plain.status[0].item()) == int(hard.status[0].item()) == int(zeros.status[0].item())


def test_sample_hard_with_info_and_its_device_checks(device):
    n_users, n_items = 60, 25
    order, pos, ign = sampler_lists(n_users, n_items, 0)
    s = TripleSampler(n_users, n_items, pos, ign, device, seed=5)
    table = torch.randn(n_users + n_items, 16, device=device, generator=torch.Generator(device=device).manual_seed(2))
    batch = s.candidates.numel()                             # every user with positives, user 5 among them
    users, p, n, score, attempt, admissible = s.sample_hard(batch, table, candidates=8, with_info=True)
    assert [t.dtype for t in (users, p, n, score, attempt, admissible)] == \
        [torch.int64] * 3 + [torch.float32, torch.int32, torch.int32]
    assert all(t.shape == (batch,) and t.device == users.device for t in (p, n, score, attempt, admissible))
    assert ((admissible >= 1) & (admissible <= 8)).all() and ((attempt >= 1) & (attempt <= 256)).all()
    assert int(n[users == 5].item()) == n_users + 9                                                 # its one admissible item
    # the halves of the table are the right ones: the score is the pair's dot product (16 products of N(0, 1) values summed
    # in another order: 1e-4 is a hundred times the rounding of either sum)
    dots = lambda items: (table[users].double() * table[items].double()).sum(1)
    assert (score.double() - dots(n)).abs().max().item() <= 1e-4
    # the winner is no worse than the uniform sampler's negative: that one is its first candidate
    twin = TripleSampler(n_users, n_items, pos, ign, device, seed=5)
    u1, _, n1 = twin.sample(batch)
    assert torch.equal(u1, users) and (dots(n1) <= score.double() + 1e-4).all() and (dots(n1) < score.double() - 1e-3).any()
    with pytest.raises(ValueError, match="is on cpu"):
        s.sample_hard(8, table.cpu())
    with pytest.raises(ValueError, match="population"):
        s.sample_hard(10 ** 6, table)
    assert s.step == 1


def test_two_training_steps_on_hard_negatives(device):
    """The autograd route on a 200-user graph, negatives from the propagated table: finite losses, clean status words and no
    negative inside its user's ignore set."""
    g = synth.make_bipartite(200, 60, 1500, seed=0)
    ei, ew = g.coo(device)
    n_users, n_items = g.n_users, g.n_items
    sampler = TripleSampler.from_pairs(n_users, n_items, g.user, g.item + n_users, g.user, g.item + n_users, device, seed=0)
    torch.manual_seed(0)
    model = lg.LightGCN(g.num_nodes, 64, 3).to(device)
    opt = torch.optim.Adam(model.parameters(), 0.005)
    owned = set(zip(g.user.tolist(), (g.item + n_users).tolist()))
    for step in range(2):
        with torch.no_grad():
            table = model.get_embedding(ei, ew) if step else model.embedding.weight.detach()
        users, pos, neg, score, attempt, admissible = sampler.sample_hard(128, table, candidates=8, with_info=True)
        opt.zero_grad()
        labels = torch.stack((torch.cat([users, users]), torch.cat([pos, neg])))
        out = model(ei, labels, ew)
        loss = model.recommendation_loss(out[:128], out[128:], 0) * 128
        loss.backward()
        opt.step()
        assert torch.isfinite(loss).item() and torch.isfinite(score).all()
        assert (admissible == 8).all() and ((neg >= n_users) & (neg < n_users + n_items)).all()
        assert not owned & set(zip(users.tolist(), neg.tolist()))
        assert owned >= set(zip(users.tolist(), pos.tolist()))
    sampler.check()
    lg.check_index_status()
