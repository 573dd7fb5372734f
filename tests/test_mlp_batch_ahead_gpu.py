"""Batch ahead on an MI355X: the backward launch publishes the next step's batch into the other
half of the parity double buffers ``xa`` / ``ya`` and the forward reads its X rows from there.

Kernel level, at M = 20, K = 80, N = 24, C = 10 over a 50-row dataset (partial last m- and n-tile,
waves with an empty K range, batches that straddle the end of the permutation) and at the
workload's 100 / 784 / 500 / 10 (49 k-steps split unevenly over 8 waves), both parities, named at
launch and taken from the counter, Adam and gradient mode. Trainer level against the gathering
path (``batch_ahead=False``) with the criterion of ``test_graph_replay_equals_eager``.

``H`` from ``xa`` is asserted bit-equal to the gathering fast path's ``H`` (same rows, same K
split, same sum order), and ``reference.py``'s twin bit-equal to its own gathering path; between
kernel and ``reference.py`` ``H`` carries the tolerance ``tests/test_mlp_step_paths_gpu.py`` uses
for the same pair, because the reference sums each dot product in torch's matmul order, not in
the kernel's (8 waves x 4 chains): neither path was ever bit-equal to it.
"""
import pytest
import torch

from arena_amd.models.mlp import FusedMLPTrainer, MLPConfig
from arena_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

# (M, K, N, C, dataset rows)
SHAPES = {"small": (20, 80, 24, 10, 50), "mnist": (100, 784, 500, 10, 250)}
# step t, parity argument: counter 2 -> step 1 (half 1; publishes batch 2, which straddles the
# end of the 50-row permutation), counter 3 -> step 2 (half 0; reads that straddling batch)
STEPS = [(1, -1), (1, 1), (2, -1), (2, 0)]
XSENT, YSENT = 0xAB, -7


def _ext():
    from arena_amd.ops import _ext
    return _ext.load()


def _close(a, b, rtol, atol, what=""):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), rtol=rtol, atol=atol,
                               msg=lambda m: f"{what}: {m}")


@pytest.fixture(scope="module")
def pools(cuda):
    """Per shape: random source material, generated once, never written."""
    out = {}
    for name, (M, K, N, C, R) in SHAPES.items():
        g = torch.Generator().manual_seed(len(name) * 1000 + M)
        p = {"x": torch.randint(0, 256, (R, K), generator=g, dtype=torch.uint8).to(cuda),
             "y": torch.randint(0, C, (R,), generator=g, dtype=torch.uint8).to(cuda),
             "perm": torch.randperm(R, generator=g).to(torch.int32).to(cuda),
             "W1": (torch.randn(N, K, generator=g) * 0.05).to(cuda),
             "b1": (torch.randn(N, generator=g) * 0.1).to(cuda),
             "W2": (torch.randn(C, N, generator=g) * 0.1).to(cuda),
             "b2": (torch.randn(C, generator=g) * 0.1).to(cuda),
             "H": torch.relu(torch.randn(M, N, generator=g)).to(cuda),
             "lg": torch.randn(M, C, generator=g).to(cuda)}
        p["H"][p["H"] < 0.3] = 0.0
        out[name] = p
    return out


def _batch(p, t, M):
    """Rows and labels of batch t: x[perm[(t * M + r) % len]]."""
    L = p["perm"].numel()
    rows = p["perm"][(t * M + torch.arange(M, device=p["perm"].device)) % L].to(torch.int64)
    return p["x"][rows], p["y"][rows].to(torch.int32)


def _pair(p, t, M, K, cuda):
    """xa / ya with batch t in half t & 1 and sentinels in the other half."""
    xa = torch.full((2, M, K), XSENT, dtype=torch.uint8, device=cuda)
    ya = torch.full((2, M), YSENT, dtype=torch.int32, device=cuda)
    xa[t & 1], ya[t & 1] = _batch(p, t, M)
    return xa, ya


def _backward(impl, p, shape, cuda, mode, t, parity, x0, labels, nxt):
    """One head-mode backward launch at step t; ``nxt`` = (next_xa, next_ya) or None."""
    M, K, N, C, _ = shape
    cur = torch.tensor([t + 1], dtype=torch.int64, device=cuda)   # B counter: step + 1
    lg2 = torch.full((2, M, C), 7.0, device=cuda)
    lg2[t & 1] = p["lg"]
    W1, W2, b1, b2 = p["W1"].clone(), p["W2"].clone(), p["b1"].clone(), p["b2"].clone()
    st = [torch.full_like(v, 1e-3) for v in (W1, W2, b1, b2)] + \
         [torch.full_like(v, 1e-4) for v in (W1, W2, b1, b2)]
    la = torch.zeros(8, device=cuda)
    ca = torch.zeros(8, dtype=torch.int32, device=cuda)
    args = ([x0, p["H"]], [1 / 255.0, 1.0], [False, False], None, None, -1, M, [None, None],
            [2, 1], [p["W2"], None], [p["H"], None], 0.9, lg2, cur, -1, p["b2"], labels, 1.0 / M,
            la, ca, mode, [W1, W2], [b1, b2], [st[0], st[1]], [st[4], st[5]], [st[2], st[3]],
            [st[6], st[7]], 1e-3, None, 0.9, 0.999, 1e-8, 0.0, cur, 1.0, False, None, None, 0)
    tail = (nxt[0], nxt[1], parity, p["x"], p["y"], p["perm"]) if nxt else (None, None, parity)
    (_ext() if impl == "hip" else ref).wgrad_grouped(*args, *tail)
    return [W1, W2, b1, b2, la, lg2] + st


@pytest.mark.parametrize("t,parity", STEPS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_publishes_next_batch(cuda, pools, name, mode, t, parity):
    p, shape = pools[name], SHAPES[name]
    M, K = shape[0], shape[1]
    xa, ya = _pair(p, t, M, K, cuda)
    keep_x, keep_y = xa[t & 1].clone(), ya[t & 1].clone()
    got = _backward("hip", p, shape, cuda, mode, t, parity, xa, ya, (xa, ya))
    torch.cuda.synchronize()
    nx, ny = _batch(p, t + 1, M)
    assert torch.equal(xa[(t + 1) & 1], nx), "published rows"
    assert torch.equal(ya[(t + 1) & 1], ny), "published labels"
    assert torch.equal(xa[t & 1], keep_x) and torch.equal(ya[t & 1], keep_y), "this step's half"
    # the same launch on a plain [M, K] batch (what the forward used to publish): identical bits
    plain = _backward("hip", p, shape, cuda, mode, t, parity, keep_x, keep_y, None)
    for a, b in zip(got, plain):
        assert torch.equal(a, b), "parity pair against the plain batch"
    # the reference twin, publishing into its own pair
    rxa, rya = _pair(p, t, M, K, cuda)
    want = _backward("ref", p, shape, cuda, mode, t, parity, rxa, rya, (rxa, rya))
    assert torch.equal(rxa, xa) and torch.equal(rya, ya), "reference twin's pair"
    for a, b, nm in zip(got[:4], want[:4], ("W1", "W2", "b1", "b2")):
        _close(a, b, 2e-4, 1e-6, nm)
    if mode == 1:
        for a, b in zip(got[6:], want[6:]):
            _close(a, b, 2e-4, 1e-6, "adam state")
    _close(got[4], want[4], 1e-4, 1e-5, "loss history")


def _forward(impl, p, shape, cuda, t, how, parity=-1):
    """One forward launch at step t. how: "gather" (idx / cursor, publishing xb / yb) or "xa"."""
    M, K, N, C, _ = shape
    A = torch.tensor([t], dtype=torch.int64, device=cuda)
    Bc = torch.zeros(1, dtype=torch.int64, device=cuda)
    H = torch.empty(M, N, device=cuda)
    w2c = torch.empty(C, N, device=cuda)
    lg2 = torch.full((2, M, C), 7.0, device=cuda)
    lg2[t & 1] = 0.0
    W1, b1, W2 = p["W1"], p["b1"], p["W2"]
    if how == "gather":
        xb = torch.zeros(M, K, dtype=torch.uint8, device=cuda)
        yb = torch.zeros(M, dtype=torch.int32, device=cuda)
        args = (p["x"], 1 / 255.0, p["perm"], A, M, W1, b1, H, 0.9, 77, A, W2, w2c, lg2, xb,
                p["y"], yb, Bc, A, 1, None)
    else:
        xa, _ = _pair(p, t, M, K, cuda)
        args = (p["x"], 1 / 255.0, None, None, 0, W1, b1, H, 0.9, 77, A, W2, w2c, lg2, None, None,
                None, Bc, A, 1, xa, parity)
    (_ext() if impl == "hip" else ref).mlp_fwd_logits(*args)
    return H, lg2, Bc, w2c


@pytest.fixture(scope="module")
def fwd_refs(cuda, pools):
    """Per shape and step: the gathering fast path's and reference.py's results, computed once."""
    out = {}
    for name, shape in SHAPES.items():
        for t in (1, 2):
            out[name, t] = (_forward("hip", pools[name], shape, cuda, t, "gather"),
                            _forward("ref", pools[name], shape, cuda, t, "gather"))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("t,parity", STEPS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_reads_published_batch(cuda, pools, fwd_refs, name, t, parity):
    p, shape = pools[name], SHAPES[name]
    H, lg2, Bc, w2c = _forward("hip", p, shape, cuda, t, "xa", parity)
    torch.cuda.synchronize()
    (gH, glg2, gBc, gw2c), (rH, rlg2, _, _) = fwd_refs[name, t]
    assert torch.equal(H, gH), f"H against the gathering fast path: {float((H - gH).abs().max())}"
    tH = _forward("ref", p, shape, cuda, t, "xa", parity)[0]
    assert torch.equal(tH, rH), "reference.py: xa twin against its gathering path"
    _close(H, rH, 1e-4, 1e-5, "H against reference.py")
    _close(lg2[t & 1], rlg2[t & 1], 1e-4, 1e-4, "logits against reference.py")
    _close(lg2[t & 1], glg2[t & 1], 1e-4, 1e-4, "logits against the gathering fast path")
    other = lg2[(t + 1) & 1]
    assert torch.equal(other, torch.full_like(other, 7.0))
    assert int(Bc) == t + 1 and int(gBc) == t + 1
    assert torch.equal(w2c, gw2c)


def test_forward_refuses_shapes_outside_the_step_kernel(cuda):
    """K > 1024 and an fp32 source have no kernel that reads xa: the binding says so."""
    M, N, C = 4, 16, 10
    A = torch.zeros(1, dtype=torch.int64, device=cuda)
    Bc = torch.zeros(1, dtype=torch.int64, device=cuda)
    for K, dt in ((1040, torch.uint8), (80, torch.float32)):
        x = torch.zeros(8, K, dtype=dt, device=cuda)
        xa = torch.zeros(2, M, K, dtype=torch.uint8, device=cuda)
        with pytest.raises(RuntimeError, match="published batch"):
            _ext().mlp_fwd_logits(x, 1 / 255.0, None, None, 0, torch.zeros(N, K, device=cuda),
                                  torch.zeros(N, device=cuda), torch.empty(M, N, device=cuda), 0.9,
                                  1, A, torch.zeros(C, N, device=cuda), None,
                                  torch.zeros(2, M, C, device=cuda), None, None, None, Bc, A, 1,
                                  xa, 0)


# ------------------------------------------------------------------------------------------------
# trainer level
# ------------------------------------------------------------------------------------------------
N_SAMPLES, B, NSTEPS = 2000, 100, 45
FUSED_STATE = ("P", "M", "V", "ctrA", "ctrB", "logits2", "rows", "loss_hist", "corr_hist", "perm")


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    return (torch.randint(0, 256, (N_SAMPLES, 784), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (N_SAMPLES,), generator=g, dtype=torch.uint8))


def _trainer(data, cuda, ahead):
    tr = FusedMLPTrainer(MLPConfig(batch=B, seed=5), data[0], data[1], device=cuda,
                         batch_ahead=ahead)
    assert tr.batch_ahead == ahead
    return tr


@pytest.fixture(scope="module")
def base(data, cuda):
    """The gathering path, eager: its first epoch order, Hbuf after step 1 and P after 45 steps.
    Computed once, never written."""
    tr = _trainer(data, cuda, False)
    perm0 = tr.perm.clone()
    tr.train_steps(1)
    h1 = tr.Hbuf.clone()
    tr.train_steps(NSTEPS - 1)
    torch.cuda.synchronize()
    return {"perm0": perm0, "h1": h1, "P": tr.P.clone()}


def _same_training(a_P, b_P, lr, steps):
    """test_graph_replay_equals_eager's criterion, its max bound (20 lr for 20 steps: Adam moves a
    parameter by at most lr per step) scaled to the steps taken."""
    diff = (a_P - b_P).abs()
    off = diff > (1e-6 + 1e-4 * b_P.abs())
    assert float(off.float().mean()) < 1e-4, int(off.sum())
    assert float(diff.max()) < 20 * lr * (steps / 20), float(diff.max())


@pytest.mark.parametrize("how", ["eager", "graph10", "graph5"])
def test_trainer_equals_gathering_path(cuda, data, base, how):
    tr = _trainer(data, cuda, True)
    assert torch.equal(tr.perm, base["perm0"])     # same seed, same epoch order
    if how == "eager":
        tr.train_steps(1)
        assert torch.equal(tr.Hbuf, base["h1"]), "Hbuf after the first step"
        tr.train_steps(NSTEPS - 1)
        assert tr.graph_steps == 0
    elif how == "graph10":                         # even length: parity baked into the launches
        assert tr.enable_graphs(10)
        assert tr._graph_static
        tr.train_steps(NSTEPS)
        assert tr.graph_steps == 40
    else:                                          # odd length: parity from the counter
        tr.train_steps(1)
        assert torch.equal(tr.Hbuf, base["h1"]), "Hbuf after the first step"
        assert tr.enable_graphs(5)
        assert not tr._graph_static
        tr.train_steps(NSTEPS - 1)
        assert tr.graph_steps == 40                # 15 + 20 + 5: epochs end at steps 20 and 40
    torch.cuda.synchronize()
    assert int(tr.ctrA.item()) == NSTEPS
    _same_training(tr.P, base["P"], tr.cfg.lr, NSTEPS)


def test_dump_outputs_scenario(cuda, data, base):
    """Snapshot the ten named tensors, steps_done and the generator; 30 steps; restore by
    attribute (xa / ya are unknown to the restorer); one step: the first step's Hbuf again."""
    tr = _trainer(data, cuda, True)
    assert tr.enable_graphs(10)
    snap = {n: getattr(tr, n).clone() for n in FUSED_STATE}
    steps_done, rng = tr.steps_done, tr._gen.get_state()
    tr.train_steps(30)
    torch.cuda.synchronize()
    for n, v in snap.items():
        getattr(tr, n).copy_(v)
    tr.steps_done = steps_done
    tr._gen.set_state(rng)
    tr.train_steps(1)
    torch.cuda.synchronize()
    assert torch.equal(tr.Hbuf, base["h1"])


def test_resume_mid_epoch(cuda, data):
    """state_dict at step 27 (epoch 2, step 7) into a fresh trainer: its next Hbuf is the
    uninterrupted run's (the saving trainer's own next step: same parameter bits)."""
    tr = _trainer(data, cuda, True)
    tr.train_steps(27)
    sd = tr.state_dict()
    tr.train_steps(1)
    want = tr.Hbuf.clone()
    tr2 = _trainer(data, cuda, True)
    tr2.train_steps(2)
    tr2.load_state_dict(sd)
    tr2.train_steps(1)
    torch.cuda.synchronize()
    assert torch.equal(tr2.Hbuf, want)
