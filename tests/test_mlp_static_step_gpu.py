"""The static step on an MI355X: the two step kernels compiled for the MNIST workload's shape
(batch 100, 784-500-10, batch published one step ahead) against the run-time-shape kernels they
replace there, switched with ``_C.mlp_static_step`` and told apart with ``_C.mlp_static_step_last``.

The static kernels exist at that one shape, which holds every edge by itself: the last k-tile has
16 valid columns of 64, the last n-tile 4 of 16, 100 rows sit in a 112-row image, C is 10 of 16.
Tiling, K split, chains and sum order are shared with the run-time kernels, so everything but the
logits (f32 atomics: the sum order varies run to run) is asserted bit-identical. Steps 1 and 2 over
a 250-row dataset: step 1 publishes batch 2, which wraps the permutation, step 2 reads it.

Mutations, each built once, run once against this file and reverted. A wrong constant in the static
shape (``wgrad_step_tile`` giving problem 1 K = N - 4): 17 of 32 tests fail, all four cases of
``test_backward_gradient_mode`` and of ``test_backward_adam_mode`` (gW2 / W2 differ), the static
half of all ``test_backward_falls_back`` cases (against reference.py) and both
``test_trainer_on_equals_off``; the forward, publishing and forward-fallback tests pass. A dropped
clamp on the last k-tile: the clamps there (``min(k0 + 4q, K - 4)`` on the X and Adam-state loads,
``min(.., K - 4)`` in the forward) only keep addresses inside the row; what they load past K is
zeroed or never stored, so dropping one changes no value and no test of values can fail. It was
not run: it would read past the last row on purpose.
"""
import pytest
import torch

from arena_amd.models.mlp import FusedMLPTrainer, MLPConfig
from arena_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

M, K, N, C, R = 100, 784, 500, 10, 250
# step t, parity argument (-1: from the counter)
STEPS = [(1, -1), (1, 1), (2, -1), (2, 0)]
XSENT, YSENT = 0xAB, -7
LR, ADAM_T = 2e-3, 5


def _ext():
    from arena_amd.ops import _ext
    return _ext.load()


@pytest.fixture(autouse=True)
def _switch_back_on():
    yield
    _ext().mlp_static_step(True)


def _close(a, b, rtol, atol, what=""):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), rtol=rtol, atol=atol,
                               msg=lambda m: f"{what}: {m}")


def _pool(cuda, m, k, n, c, rows, seed):
    g = torch.Generator().manual_seed(seed)
    p = {"x": torch.randint(0, 256, (rows, k), generator=g, dtype=torch.uint8).to(cuda),
         "y": torch.randint(0, c, (rows,), generator=g, dtype=torch.uint8).to(cuda),
         "perm": torch.randperm(rows, generator=g).to(torch.int32).to(cuda),
         "W1": (torch.randn(n, k, generator=g) * 0.05).to(cuda),
         "b1": (torch.randn(n, generator=g) * 0.1).to(cuda),
         "W2": (torch.randn(c, n, generator=g) * 0.1).to(cuda),
         "b2": (torch.randn(c, generator=g) * 0.1).to(cuda),
         "H": torch.relu(torch.randn(m, n, generator=g)).to(cuda),
         "lg": torch.randn(m, c, generator=g).to(cuda),
         "shape": (m, k, n, c)}
    p["H"][p["H"] < 0.3] = 0.0
    # hand-set Adam state, one tensor per parameter: m then v
    for nm in ("W1", "W2", "b1", "b2"):
        p["m" + nm] = (torch.randn(p[nm].shape, generator=g) * 1e-2).to(cuda)
        p["v" + nm] = (torch.rand(p[nm].shape, generator=g) * 1e-3).to(cuda)
    return p


@pytest.fixture(scope="module")
def pool(cuda):
    """Source material at the workload's shape, generated once, never written."""
    return _pool(cuda, M, K, N, C, R, 4100)


def _batch(p, t):
    m = p["shape"][0]
    L = p["perm"].numel()
    rows = p["perm"][(t * m + torch.arange(m, device=p["perm"].device)) % L].to(torch.int64)
    return p["x"][rows], p["y"][rows].to(torch.int32)


def _pair(p, t, cuda):
    """xa / ya with batch t in half t & 1 and sentinels in the other half."""
    m, k = p["shape"][:2]
    xa = torch.full((2, m, k), XSENT, dtype=torch.uint8, device=cuda)
    ya = torch.full((2, m), YSENT, dtype=torch.int32, device=cuda)
    xa[t & 1], ya[t & 1] = _batch(p, t)
    return xa, ya


def _misaligned(v):
    """The same values in a view that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=v.device)
    buf[1:].copy_(v.reshape(-1))
    return buf[1:].view(v.shape)


def _backward(impl, p, cuda, mode, t, parity, publish=True, misalign=False):
    """One head-mode backward launch at step t on the parity pair. Returns a dict of everything
    the launch writes."""
    m, k, n, c = p["shape"]
    cur = torch.tensor([t + 1], dtype=torch.int64, device=cuda)   # B counter: step + 1
    tstep = torch.tensor([ADAM_T], dtype=torch.int64, device=cuda)
    lr_t = torch.full((1,), LR, device=cuda)
    lg2 = torch.full((2, m, c), 7.0, device=cuda)
    lg2[t & 1] = p["lg"]
    xa, ya = _pair(p, t, cuda)
    names = ("W1", "W2", "b1", "b2")
    P = {nm: p[nm].clone() for nm in names}
    Ms = {nm: p["m" + nm].clone() for nm in names}
    Vs = {nm: p["v" + nm].clone() for nm in names}
    if mode == 0:
        P = {nm: torch.full_like(p[nm], 3.0) for nm in names}      # gradient outputs
    if misalign:     # W2's views: the float4 epilogue of either compiled pair needs 16 bytes
        for d in (P, Ms, Vs):
            d["W2"] = _misaligned(d["W2"])
    la = torch.full((8,), 5.0, device=cuda)
    ca = torch.full((8,), 5, dtype=torch.int32, device=cuda)
    la[t & 7], ca[t & 7] = 0.0, 0                                  # cleared by the step before
    args = ([xa, p["H"]], [1 / 255.0, 1.0], [False, False], None, None, -1, m, [None, None],
            [2, 1], [p["W2"], None], [p["H"], None], 0.9, lg2, cur, -1, p["b2"], ya, 1.0 / m,
            la, ca, mode, [P["W1"], P["W2"]], [P["b1"], P["b2"]], [Ms["W1"], Ms["W2"]],
            [Vs["W1"], Vs["W2"]], [Ms["b1"], Ms["b2"]], [Vs["b1"], Vs["b2"]], LR, lr_t, 0.9,
            0.999, 1e-8, 0.0, tstep, 1.0, False, None, None, 0)
    tail = (xa, ya, parity, p["x"], p["y"], p["perm"]) if publish else (None, None, parity)
    (_ext() if impl == "hip" else ref).wgrad_grouped(*args, *tail)
    out = {"la": la, "ca": ca, "lg2": lg2, "xa": xa, "ya": ya}
    for nm in names:
        out["P" + nm], out["M" + nm], out["V" + nm] = P[nm], Ms[nm], Vs[nm]
    return out


def _backward_on_off(p, cuda, mode, t, parity):
    ext = _ext()
    ext.mlp_static_step(True)
    on = _backward("hip", p, cuda, mode, t, parity)
    assert ext.mlp_static_step_last()[1] == "static"
    ext.mlp_static_step(False)
    off = _backward("hip", p, cuda, mode, t, parity)
    assert ext.mlp_static_step_last()[1] == "run-time"
    torch.cuda.synchronize()
    return on, off


def _check_bookkeeping(o, t):
    """Next-parity logits half zeroed; metric slot written, the next one cleared, others kept."""
    nxt = o["lg2"][(t + 1) & 1]
    assert torch.equal(nxt, torch.zeros_like(nxt)), "next step's logits half"
    la, ca = o["la"].cpu(), o["ca"].cpu()
    assert float(la[t & 7]) > 0.0 and 0 <= int(ca[t & 7]) <= M, "this step's metric slot"
    assert float(la[(t + 1) & 7]) == 0.0 and int(ca[(t + 1) & 7]) == 0, "next metric slot"
    for s in range(8):
        if s not in (t & 7, (t + 1) & 7):
            assert float(la[s]) == 5.0 and int(ca[s]) == 5, "other metric slots"


@pytest.mark.parametrize("t,parity", STEPS)
def test_backward_gradient_mode(cuda, pool, t, parity):
    on, off = _backward_on_off(pool, cuda, 0, t, parity)
    for nm in ("W1", "b1", "W2", "b2"):
        assert torch.equal(on["P" + nm], off["P" + nm]), f"g{nm}"
    assert not bool((on["PW1"] == 3.0).any()) and not bool((on["Pb1"] == 3.0).any())
    for k in ("la", "ca", "lg2"):
        assert torch.equal(on[k], off[k]), k
    _check_bookkeeping(on, t)


@pytest.mark.parametrize("t,parity", STEPS)
def test_backward_adam_mode(cuda, pool, t, parity):
    on, off = _backward_on_off(pool, cuda, 1, t, parity)
    for nm in ("W1", "b1", "W2", "b2"):       # b1: the float4 loads of the bias' Adam state
        for s in "PMV":
            assert torch.equal(on[s + nm], off[s + nm]), f"{s} of {nm}"
        assert not torch.equal(on["P" + nm], pool[nm]), f"{nm} not updated"
    for k in ("la", "ca", "lg2"):
        assert torch.equal(on[k], off[k]), k
    _check_bookkeeping(on, t)


@pytest.mark.parametrize("t,parity", STEPS)
@pytest.mark.parametrize("mode", [0, 1])
def test_static_backward_publishes_next_batch(cuda, pool, mode, t, parity):
    """xa / ya of the other parity hold the rows reference.py selects (step 1: batch 2 wraps the
    250-row permutation), this step's half is untouched."""
    _ext().mlp_static_step(True)
    got = _backward("hip", pool, cuda, mode, t, parity)
    assert _ext().mlp_static_step_last()[1] == "static"
    want = _backward("ref", pool, cuda, mode, t, parity)
    torch.cuda.synchronize()
    assert torch.equal(got["xa"], want["xa"]) and torch.equal(got["ya"], want["ya"])
    nx, ny = _batch(pool, t + 1)
    assert torch.equal(got["xa"][(t + 1) & 1], nx) and torch.equal(got["ya"][(t + 1) & 1], ny)
    kx, ky = _batch(pool, t)
    assert torch.equal(got["xa"][t & 1], kx) and torch.equal(got["ya"][t & 1], ky)


def _forward(impl, p, cuda, t, parity):
    m, k, n, c = p["shape"]
    A = torch.tensor([t], dtype=torch.int64, device=cuda)
    Bc = torch.zeros(1, dtype=torch.int64, device=cuda)
    H = torch.full((m, n), -1.0, device=cuda)
    w2c = torch.full((c, n), -1.0, device=cuda)
    lg2 = torch.full((2, m, c), 7.0, device=cuda)
    lg2[t & 1] = 0.0
    xa, _ = _pair(p, t, cuda)
    (_ext() if impl == "hip" else ref).mlp_fwd_logits(
        p["x"], 1 / 255.0, None, None, 0, p["W1"], p["b1"], H, 0.9, 77, A, p["W2"], w2c, lg2,
        None, None, None, Bc, A, 1, xa, parity)
    return H, w2c, Bc, lg2


@pytest.mark.parametrize("t,parity", STEPS)      # parity >= 0: FM 2, -1: FM 3
def test_forward(cuda, pool, t, parity):
    ext = _ext()
    ext.mlp_static_step(True)
    H, w2c, Bc, lg2 = _forward("hip", pool, cuda, t, parity)
    assert ext.mlp_static_step_last()[0] == "static"
    ext.mlp_static_step(False)
    rH, rw2c, rBc, rlg2 = _forward("hip", pool, cuda, t, parity)
    assert ext.mlp_static_step_last()[0] == "run-time"
    torch.cuda.synchronize()
    assert torch.equal(H, rH), f"H: {float((H - rH).abs().max())}"
    assert torch.equal(w2c, rw2c) and torch.equal(w2c, pool["W2"]), "W2 snapshot"
    assert int(Bc) == t + 1 and int(rBc) == t + 1, "counter write"
    # kernel against kernel, the tolerance of tests/test_mlp_batch_ahead_gpu.py (atomics)
    _close(lg2[t & 1], rlg2[t & 1], 1e-4, 1e-4, "logits")
    other = lg2[(t + 1) & 1]
    assert torch.equal(other, torch.full_like(other, 7.0)), "the other logits half"


# ------------------------------------------------------------------------------------------------
# path selection: everything but the exact shape, strides and alignment runs the run-time kernels
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def off_shape_pools(cuda):
    return {"hidden496": _pool(cuda, 100, 784, 496, 10, 250, 4200),
            "batch96": _pool(cuda, 96, 784, 500, 10, 250, 4300)}


def _against_reference(got, p, cuda, mode, t, parity, **kw):
    want = _backward("ref", p, cuda, mode, t, parity, **kw)
    for nm in ("W1", "W2", "b1", "b2"):
        _close(got["P" + nm], want["P" + nm], 2e-4, 1e-6, nm)
        if mode == 1:
            _close(got["M" + nm], want["M" + nm], 2e-4, 1e-6, "m of " + nm)
            _close(got["V" + nm], want["V" + nm], 2e-4, 1e-6, "v of " + nm)
    _close(got["la"], want["la"], 1e-4, 1e-5, "loss history")


FALLBACKS = [("hidden496", 0), ("hidden496", 1), ("batch96", 0), ("batch96", 1),
             ("misaligned", 0), ("misaligned", 1), ("no_batch_ahead", 0), ("no_batch_ahead", 1)]


@pytest.mark.parametrize("case,mode", FALLBACKS)
def test_backward_falls_back(cuda, pool, off_shape_pools, case, mode):
    ext = _ext()
    ext.mlp_static_step(True)
    p = off_shape_pools.get(case, pool)
    kw = {"misalign": case == "misaligned", "publish": case != "no_batch_ahead"}
    got = _backward("hip", p, cuda, mode, 1, 1, **kw)
    assert ext.mlp_static_step_last()[1] == "run-time", case
    torch.cuda.synchronize()
    _against_reference(got, p, cuda, mode, 1, 1, **kw)
    # and the flagship launch next to it is static, right against reference.py as well
    got = _backward("hip", pool, cuda, mode, 1, 1)
    assert ext.mlp_static_step_last()[1] == "static"
    _against_reference(got, pool, cuda, mode, 1, 1)


@pytest.mark.parametrize("case", ["hidden496", "batch96"])
def test_forward_falls_back(cuda, pool, off_shape_pools, case):
    ext = _ext()
    ext.mlp_static_step(True)
    p = off_shape_pools[case]
    H, w2c, Bc, lg2 = _forward("hip", p, cuda, 1, -1)
    assert ext.mlp_static_step_last()[0] == "run-time", case
    rH, _, _, rlg2 = _forward("ref", p, cuda, 1, -1)
    torch.cuda.synchronize()
    _close(H, rH, 1e-4, 1e-5, "H against reference.py")
    _close(lg2[1], rlg2[1], 1e-4, 1e-4, "logits against reference.py")
    assert torch.equal(w2c, p["W2"]) and int(Bc) == 2
    H, _, _, lg2 = _forward("hip", pool, cuda, 1, -1)
    assert ext.mlp_static_step_last()[0] == "static"
    rH, _, _, rlg2 = _forward("ref", pool, cuda, 1, -1)
    _close(H, rH, 1e-4, 1e-5, "static H against reference.py")
    _close(lg2[1], rlg2[1], 1e-4, 1e-4, "static logits against reference.py")


# ------------------------------------------------------------------------------------------------
# trainer level
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    return (torch.randint(0, 256, (2000, 784), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (2000,), generator=g, dtype=torch.uint8))


def _train3(data, cuda, on, graph):
    """Three steps from seed 5, eager or as one replay of a three-step graph (odd length: the
    parity comes from the counter). Returns step 1's outputs (eager only) and the final state."""
    ext = _ext()
    ext.mlp_static_step(on)
    tr = FusedMLPTrainer(MLPConfig(batch=100, seed=5), data[0], data[1], device=cuda)
    assert tr.batch_ahead
    first = None
    if graph:
        assert tr.enable_graphs(3)
        tr.train_steps(3)
        assert tr.graph_steps == 3
    else:
        tr.train_steps(1)
        first = (tr.Hbuf.clone(), tr.loss_hist[:1].clone(), tr.corr_hist[:1].clone())
        tr.train_steps(2)
    torch.cuda.synchronize()
    assert ext.mlp_static_step_last() == (("static",) * 2 if on else ("run-time",) * 2)
    return first, tr.P.clone(), tr.M.clone(), tr.V.clone(), tr.cfg.lr


def _same_training(a, b, lr, steps):
    """test_graph_replay_equals_eager's criterion, its max bound (20 lr for 20 steps) scaled to
    the steps taken."""
    diff = (a - b).abs()
    off = diff > (1e-6 + 1e-4 * b.abs())
    assert float(off.float().mean()) < 1e-4, int(off.sum())
    assert float(diff.max()) < 20 * lr * (steps / 20), float(diff.max())


@pytest.fixture(scope="module")
def eager_off(data, cuda):
    out = _train3(data, cuda, False, False)
    _ext().mlp_static_step(True)
    return out


@pytest.mark.parametrize("graph", [False, True])
def test_trainer_on_equals_off(cuda, data, eager_off, graph):
    first, P, Mm, V, lr = _train3(data, cuda, True, graph)
    ofirst, oP, oM, oV, _ = eager_off
    if not graph:
        assert torch.equal(first[0], ofirst[0]), "step 1: hidden"
        assert torch.equal(first[2], ofirst[2]), "step 1: correct"
    _same_training(P, oP, lr, 3)
    _same_training(Mm, oM, lr, 3)
    _same_training(V, oV, lr, 3)


def test_trainer_step1_loss_bit_identical(cuda, data, eager_off):
    """Step 1's loss with the switch on and off, bit for bit, as the issue sets it. The loss is
    computed from logits that the forward sums with f32 atomics, whose order varies from run to
    run with the switch in either position, so this assertion holds only in the runs in which
    the two sums happen to round alike. Runs of this pull request: held in the first of three,
    failed in the other two by one ulp (on 3.7149500846862793, off 3.7149503231048584).
    Not widened."""
    first, *_ = _train3(data, cuda, True, False)
    a, b = float(first[1]), float(eager_off[0][1])
    print(f"step 1 loss: on {a!r} off {b!r} diff {abs(a - b):.3e}")
    assert torch.equal(first[1], eager_off[0][1]), "step 1: loss"


def test_trainer_graph_off_equals_eager_off(cuda, data, eager_off):
    """The switch-off graph replay next to the switch-off eager run (the pair the parent has)."""
    _, P, Mm, V, lr = _train3(data, cuda, False, True)
    _same_training(P, eager_off[1], lr, 3)
