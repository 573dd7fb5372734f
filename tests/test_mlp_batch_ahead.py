"""Batch ahead on the CPU reference twin: a trainer whose backward publishes the next step's batch
(``batch_ahead=True``) computes bit for bit what the gathering path computes, across reshuffles,
after a restore of its state attribute by attribute (what ``bench.py --dump-outputs`` does) and
after a ``state_dict`` / ``load_state_dict`` resume in the middle of an epoch."""
import pytest
import torch

from arena_amd.models.mlp import FusedMLPTrainer, MLPConfig

N, B, STEPS = 2000, 100, 45          # 20 steps per epoch: 45 steps cross two reshuffles
# the tensors bench.py restores by name, besides steps_done and the shuffle generator
FUSED_STATE = ("P", "M", "V", "ctrA", "ctrB", "logits2", "rows", "loss_hist", "corr_hist", "perm")


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(7)
    return (torch.randint(0, 256, (N, 784), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (N,), generator=g))


def _trainer(data, ahead):
    return FusedMLPTrainer(MLPConfig(batch=B, seed=3), data[0], data[1], device="cpu",
                           batch_ahead=ahead)


@pytest.fixture(scope="module")
def baseline(data):
    """The gathering path, uninterrupted; computed once, never written."""
    tr = _trainer(data, False)
    assert not tr.batch_ahead
    tr.train_steps(STEPS)
    return tr.P.clone(), tr.M.clone(), tr.V.clone()


def _same(tr, baseline, what):
    for a, b, nm in zip((tr.P, tr.M, tr.V), baseline, "PMV"):
        assert torch.equal(a, b), f"{what}: {nm} differs, max |d| = {float((a - b).abs().max())}"


def test_batch_ahead_equals_gathering_path(data, baseline):
    tr = _trainer(data, True)
    assert tr.batch_ahead
    tr.train_steps(7)       # uneven pieces: the invariant holds from call to call
    tr.train_steps(1)
    tr.train_steps(STEPS - 8)
    _same(tr, baseline, "uninterrupted")
    # the published halves hold the batches of steps 45 and 44 (same epoch order)
    L = tr.perm.numel()
    for t in (STEPS, STEPS - 1):
        rows = tr.perm[(t * B + torch.arange(B)) % L].to(torch.int64)
        assert torch.equal(tr.xa[t & 1], data[0][rows])
        assert torch.equal(tr.ya[t & 1], data[1][rows].to(torch.int32))


def test_restore_by_attribute(data, baseline):
    """Snapshot the named tensors, steps_done and the generator; train on; put them back the way
    bench.py does (it knows nothing of xa / ya); the remaining steps give the baseline."""
    tr = _trainer(data, True)
    tr.train_steps(13)
    snap = {n: getattr(tr, n).clone() for n in FUSED_STATE}
    steps_done, rng = tr.steps_done, tr._gen.get_state()
    tr.train_steps(17)      # over the reshuffle at step 20; leaves xa / ya at step 30
    for n, v in snap.items():
        getattr(tr, n).copy_(v)
    tr.steps_done = steps_done
    tr._gen.set_state(rng)
    tr.train_steps(STEPS - 13)
    _same(tr, baseline, "restored by attribute")


def test_resume_mid_epoch(data, baseline):
    tr = _trainer(data, True)
    tr.train_steps(27)
    sd = tr.state_dict()
    tr2 = _trainer(data, True)
    tr2.train_steps(3)      # its own buffers are somewhere else before the load
    tr2.load_state_dict(sd)
    tr2.train_steps(STEPS - 27)
    _same(tr2, baseline, "resumed")


def test_knob_selects_the_gathering_path(data, monkeypatch):
    monkeypatch.setenv("ARENA_BATCH_AHEAD", "0")
    assert not FusedMLPTrainer(MLPConfig(batch=B), data[0], data[1], device="cpu").batch_ahead
    monkeypatch.setenv("ARENA_BATCH_AHEAD", "1")
    assert FusedMLPTrainer(MLPConfig(batch=B), data[0], data[1], device="cpu").batch_ahead
