"""The partitioned path over RCCL (torch.distributed backend "nccl"), one rank per GPU -- what the driver's
multi-GPU bench runs.  The two-rank tests need at least two devices, so they are skipped on the one-GPU test box and
run on the 8-GPU node; the same workers run there over gloo on one GPU (test_partition_gpu.py).  What DOES run on one
GPU: a partition of ONE rank forced through the backend (LGCN_COMM_FORCE=1) -- RCCL refuses two ranks on one device, but
a one-rank communicator is legal, and everything on torch's side of the collectives is the same: eager communicator
creation with ``device_id``, asynchronous all-reduce handles on views of the tables, ``wait()`` on the launch stream,
``all_gather_into_tensor``, the barrier, and ProcessGroupNCCL's watchdog thread working beside the HIP-graph capture of
the recorded trainer (thread-local capture mode).  Every test runs at D=64, K=3 and has a twin at the reference's D=90,
K=5."""
import pytest
import torch

from test_partition_gpu import REFERENCE_SHAPE, _check_training, _train_worker, _worker, run_ranks

pytestmark = pytest.mark.gpu


def _world():
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip(f"RCCL needs one GPU per rank; {n} device(s) visible")
    return min(n, 4)          # at most 6 processes may share a box's GPUs


def _rccl_forward(dim, layers):
    world = _world()
    results = run_ranks(_worker, world, backend="nccl", cfg=dict(dim=dim, layers=layers))
    for rank, r in results.items():
        assert r["backend"] == "nccl" and r["world"] == world
        assert r["own"] <= 1e-5 and r["items"] <= 1e-5 and r["full"] <= 1e-5 and r["worst_row"] <= 1e-5, (rank, r)
        assert r["recorded_same"], (rank, r)
    assert len({r["recorded"] for r in results.values()}) == 1          # every rank replays, or none does
    assert abs(sum(r["share"] for r in results.values()) - 1.0) < 1e-6


def test_rccl_forward_matches_single_gpu(device):
    _rccl_forward(64, 3)


@pytest.mark.parametrize("dim,layers", REFERENCE_SHAPE)
def test_rccl_forward_matches_single_gpu_at_the_reference_shape(device, dim, layers):
    _rccl_forward(dim, layers)


def _rccl_training_step(dim, layers):
    world = _world()
    results = run_ranks(_train_worker, world, backend="nccl", cfg=dict(dim=dim, layers=layers))
    for rank, r in results.items():
        assert r["backend"] == "nccl" and r["world"] == world
        assert r["bpr"] <= 1e-5 and r["reg"] <= 1e-5 and r["own"] <= 1e-5 and r["items"] <= 1e-5, (rank, r)


def test_rccl_training_step_matches_single_gpu(device):
    _rccl_training_step(64, 3)


@pytest.mark.parametrize("dim,layers", REFERENCE_SHAPE)
def test_rccl_training_step_matches_single_gpu_at_the_reference_shape(device, dim, layers):
    _rccl_training_step(dim, layers)


def _one_rank_through_rccl(monkeypatch, dim, layers):
    monkeypatch.setenv("LGCN_COMM_FORCE", "1")             # read at import time by the spawned worker
    cfg = dict(dim=dim, layers=layers)
    fwd = run_ranks(_worker, 1, backend="nccl", cfg=cfg)[0]
    assert fwd["backend"] == "nccl" and fwd["world"] == 1
    assert fwd["own"] <= 1e-5 and fwd["items"] <= 1e-5 and fwd["full"] <= 1e-5 and fwd["worst_row"] <= 1e-5, fwd
    assert fwd["recorded"] and fwd["recorded_same"], fwd    # the forward with its collectives as ONE replayed HIP graph
    r = run_ranks(_train_worker, 1, backend="nccl", cfg=cfg)[0]
    assert r["backend"] == "nccl" and r["world"] == 1
    _check_training({0: r}, full_launches=1)                 # graphs="full": ONE graph, the collectives inside


def test_one_rank_goes_through_the_rccl_process_group(device, monkeypatch):
    """Forward, both training paths, sharded Adam and the recorded trainer of a ONE-rank partition with every collective
    issued to the real backend (identities there): the same checks as the two-rank workers."""
    _one_rank_through_rccl(monkeypatch, 64, 3)


@pytest.mark.parametrize("dim,layers", REFERENCE_SHAPE)
def test_one_rank_goes_through_the_rccl_process_group_at_the_reference_shape(device, monkeypatch, dim, layers):
    """The same at D=90, K=5: the seeded backward's exchanged item blocks must be dense tensors (RCCL refuses a strided
    view of a padded table)."""
    _one_rank_through_rccl(monkeypatch, dim, layers)
