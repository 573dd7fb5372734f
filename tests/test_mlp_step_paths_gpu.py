"""The MNIST step's kernels on every code path they can take (runs on an MI355X).

Backward (``wgrad_grouped`` with the softmax head): the logits buffer named at launch or by the
counter, the per-block softmax on its edge rows, the vectorised write-through epilogue (Adam and
gradient mode) and its scalar fall-back, the chunked generic path. Forward (``mlp_fwd_logits``):
the per-tile logits partial and what it must leave untouched. All against
``arena_amd.ops.reference`` with the tolerances ``tests/test_ops_gpu.py`` uses for the same ops;
the softmax edge rows also against fp32 ``F.cross_entropy`` with the tolerance of
``tests/test_xent_head_gpu.py``.
"""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from arena_amd.models.mlp import FusedMLPTrainer, MLPConfig
from arena_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

ROWS = 300            # dataset rows behind the gather
MS = (1, 5, 100, 128, 130)
CS = (2, 10, 16)
NS = (16, 20, 36)
KS = (64, 100, 784)


def _close(a, b, rtol, atol, what=""):
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), rtol=rtol, atol=atol,
                               msg=lambda m: f"{what}: {m}")


def _ext():
    from arena_amd.ops import _ext
    return _ext.load()


@pytest.fixture(scope="module")
def pool(cuda):
    """Random source material, generated once and sliced per case (never written)."""
    g = torch.Generator().manual_seed(1234)
    p = {
        "data": {K: torch.randint(0, 256, (ROWS, K), generator=g, dtype=torch.uint8).to(cuda)
                 for K in KS},
        "labels": torch.randint(0, 16, (ROWS,), generator=g).to(cuda),
        "idx": torch.randperm(ROWS, generator=g).to(torch.int32).to(cuda),
        "H": torch.relu(torch.randn(130, 36, generator=g)).to(cuda),
        "W2c": (torch.randn(16, 36, generator=g) * 0.1).to(cuda),
        "lg": torch.randn(130, 16, generator=g).to(cuda),
        "b2": torch.randn(16, generator=g).to(cuda),
        "W1": (torch.randn(36, 784, generator=g) * 0.01).to(cuda),
        "W2": (torch.randn(16, 36, generator=g) * 0.01).to(cuda),
    }
    p["H"][p["H"] < 0.3] = 0.0
    return p


def _step_case(pool, cuda, M, C, N, K, mode, cur, parity, gather):
    """One backward launch (hidden layer through head mode 2, output layer through head mode 1)
    natively and by the reference; returns both result tuples."""
    hs = cur - 1                                   # step index: counter + head_step_off
    data = pool["data"][K]
    lab_all = (pool["labels"] % C)
    Hh = pool["H"][:M, :N].contiguous()
    W2c = pool["W2c"][:C, :N].contiguous()
    b2v = pool["b2"][:C].contiguous()
    if gather:    # dataset rows and uint8 labels behind the permutation
        x0, labels, idx = data, lab_all.to(torch.uint8), pool["idx"]
    else:         # the batch the forward published: rows in order, int32 labels
        x0, labels, idx = data[:M].contiguous(), lab_all[:M].to(torch.int32), None
    res = {}
    for impl in ("hip", "ref"):
        curt = torch.tensor([cur], dtype=torch.int64, device=cuda)
        lg2 = torch.full((2, M, C), 7.0, device=cuda)   # the other buffer must be zeroed
        lg2[hs & 1] = pool["lg"][:M, :C]
        W1 = pool["W1"][:N, :K].clone()
        W2 = pool["W2"][:C, :N].clone()
        b1 = torch.zeros(N, device=cuda)
        b2 = b2v.clone()
        st = [torch.full_like(t, 1e-3) for t in (W1, W2, b1, b2)] + \
             [torch.full_like(t, 1e-4) for t in (W1, W2, b1, b2)]
        la = torch.zeros(8, device=cuda)
        ca = torch.zeros(8, dtype=torch.int32, device=cuda)
        la[(hs + 1) & 7] = 5.0
        args = ([x0, Hh], [1 / 255.0, 1.0], [gather, False], idx, curt if gather else None, -1, M,
                [None, None], [2, 1], [W2c, None], [Hh, None], 0.9, lg2, curt, -1, b2v, labels,
                1.0 / M, la, ca, mode, [W1, W2], [b1, b2], [st[0], st[1]], [st[4], st[5]],
                [st[2], st[3]], [st[6], st[7]], 1e-3, None, 0.9, 0.999, 1e-8, 0.0, curt, 1.0,
                False, None, None, 0)
        if impl == "hip":
            _ext().wgrad_grouped(*args, None, None, parity)
        else:
            ref.wgrad_grouped(*args, None, None, parity)
        res[impl] = (W1, W2, b1, b2, la, ca, lg2, st)
    return res["hip"], res["ref"], hs


def _check_step(h, r, hs, mode, what):
    for a, b, nm in zip(h[:4], r[:4], ("W1", "W2", "b1", "b2")):
        _close(a, b, 2e-4, 1e-6, f"{what} {nm}")
    if mode == 1:
        for a, b in zip(h[7], r[7]):
            _close(a, b, 2e-4, 1e-6, f"{what} adam state")
    _close(h[4], r[4], 1e-4, 1e-5, f"{what} loss history")
    assert float(h[4][(hs + 1) & 7]) == 0.0, what          # next slot zeroed
    assert torch.equal(h[5].cpu(), r[5].cpu()), what
    assert float(h[6][(hs + 1) & 1].abs().sum()) == 0.0, what  # next logits buffer zeroed


# counter 6 -> step 5 (parity 1), counter 7 -> step 6 (parity 0); -1 reads it from the counter
@pytest.mark.parametrize("cur,parity", [(6, -1), (6, 1), (7, 0)])
@pytest.mark.parametrize("mode", [0, 1])
def test_backward_shapes(cuda, pool, mode, cur, parity):
    """Every M x C x N x K: empty 16-lane rows (M 1, 5), the second chunk (M 130), both class
    bounds with lane 15 live (C 16), partial n- and k-tiles (N 20, 36; K 100). The batch source
    alternates between the published batch and the dataset gather from case to case."""
    for i, (M, C, N, K) in enumerate(itertools.product(MS, CS, NS, KS)):
        gather = bool((i + mode + cur + parity) & 1)
        h, r, hs = _step_case(pool, cuda, M, C, N, K, mode, cur, parity, gather)
        _check_step(h, r, hs, mode, f"M{M} C{C} N{N} K{K} g{int(gather)}")


def test_backward_rejects_k_not_multiple_of_4(cuda, pool):
    """K = 70: the X staging moves 4 k per item, so the binding refuses K % 4 != 0 before any
    launch (no epilogue, vector or scalar, ever sees such a K)."""
    x = torch.zeros(8, 70, device=cuda)
    dz = torch.zeros(8, 16, device=cuda)
    W = torch.zeros(16, 70, device=cuda)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        _ext().wgrad_grouped([x], [1.0], [False], None, None, 0, 8, [dz], [0], [None], [None],
                             1.0, None, None, 0, None, None, 1.0, None, None, 0, [W], [None],
                             [None], [None], [None], [None], 1e-3, None, 0.9, 0.999, 1e-8, 0.0,
                             None, 1.0, False, None, None, 0, None, None, -1)


def _edge_logits(C):
    """Rows: a dominant class at +80 over -80; all equal; two equal maxima (labelled with the
    lower, then with the higher index); labels 0 and C-1 on ordinary rows."""
    hi = C - 1
    rows = [torch.full((C,), -80.0), torch.full((C,), 0.25), torch.full((C,), -1.0),
            torch.full((C,), -1.0), torch.linspace(-2, 2, C), torch.linspace(2, -2, C),
            torch.full((C,), 80.0), torch.zeros(C)]
    rows[0][1 % C] = 80.0
    rows[2][0] = rows[2][hi] = 3.0
    rows[3][0] = rows[3][hi] = 3.0
    rows[6][hi] = -80.0
    labels = [1 % C, 0, 0, hi, 0, hi, hi, hi]
    # correct: row 0 yes; all-equal -> class 0 yes; tie labelled low yes, labelled high no;
    # linspace up labelled 0 no; linspace down labelled C-1 no; row 6 (min at C-1) no; zeros no
    correct = 3
    return torch.stack(rows), torch.tensor(labels), correct


@pytest.mark.parametrize("C", [2, 10, 16])
@pytest.mark.parametrize("parity", [-1, 1])
def test_softmax_edge_rows(cuda, C, parity):
    """dlogits read back exactly: the output layer's input is the identity, so dW2[c][m] is
    dlogits[m][c] and db2 its column sum; loss and correct count from the history slot."""
    lg, y, correct = _edge_logits(C)
    M = lg.shape[0]
    lg, y = lg.to(cuda), y.to(cuda)
    lt = lg.clone().requires_grad_(True)
    loss_ref = F.cross_entropy(lt, y)
    loss_ref.backward()
    cur = torch.tensor([6], dtype=torch.int64, device=cuda)
    lg2 = torch.zeros(2, M, C, device=cuda)
    lg2[1] = lg
    eye = torch.eye(M, device=cuda)
    gW = torch.full((C, M), 9.0, device=cuda)
    gb = torch.full((C,), 9.0, device=cuda)
    la = torch.zeros(8, device=cuda)
    ca = torch.zeros(8, dtype=torch.int32, device=cuda)
    _ext().wgrad_grouped([eye], [1.0], [False], None, None, 0, M, [None], [1], [None], [None],
                         1.0, lg2, cur, -1, None, y.to(torch.int32), 1.0 / M, la, ca, 0, [gW],
                         [gb], [None], [None], [None], [None], 1e-3, None, 0.9, 0.999, 1e-8, 0.0,
                         None, 1.0, False, None, None, 0, None, None, parity)
    dl = gW.t()
    assert torch.allclose(dl, lt.grad, rtol=1e-5, atol=1e-7), (dl - lt.grad).abs().max()
    assert torch.allclose(gb, lt.grad.sum(0), rtol=1e-5, atol=1e-7)
    assert torch.allclose(la[5], loss_ref.detach(), rtol=1e-5, atol=1e-5), (la[5], loss_ref)
    assert int(ca[5]) == correct
    # the all-equal row alone: loss ln C, argmax class 0
    la.zero_()
    ca.zero_()
    lg2[1] = 0.25
    _ext().wgrad_grouped([eye], [1.0], [False], None, None, 0, M, [None], [1], [None], [None],
                         1.0, lg2, cur, -1, None, torch.zeros(M, dtype=torch.int32, device=cuda),
                         1.0 / M, la, ca, 0, [gW], [gb], [None], [None], [None], [None], 1e-3,
                         None, 0.9, 0.999, 1e-8, 0.0, None, 1.0, False, None, None, 0, None, None,
                         parity)
    assert abs(float(la[5]) - math.log(C)) <= 1e-5 * (1 + math.log(C))
    assert int(ca[5]) == M


@pytest.mark.parametrize("pad", [4, 1])   # 16-byte-aligned rows: float4 epilogue; else scalar
def test_adam_epilogue_padded_flat_buffer(cuda, pool, pad):
    """3 Adam steps on N=20, K=100 inside padded flat buffers: P/M/V follow the reference and
    nothing outside [N) x [K) is written."""
    M, C, N, K = 100, 10, 20, 100
    sent = 123456.0
    x0 = pool["data"][K][:M].contiguous()
    labels = (pool["labels"][:M] % C).to(torch.int32)
    Hh = pool["H"][:M, :N].contiguous()
    W2c = pool["W2c"][:C, :N].contiguous()
    b2v = pool["b2"][:C].contiguous()
    out = {}
    for impl in ("hip", "ref"):
        flats = [torch.full((pad + N * K + 7,), sent, device=cuda) for _ in range(3)]
        W1, m1, v1 = (f[pad:pad + N * K].view(N, K) for f in flats)
        W1.copy_(pool["W1"][:N, :K])
        m1.fill_(1e-3)
        v1.fill_(1e-4)
        W2 = pool["W2"][:C, :N].clone()
        b1 = torch.zeros(N, device=cuda)
        b2 = b2v.clone()
        st = [torch.full_like(t, 1e-3) for t in (W2, b1, b2)] + \
             [torch.full_like(t, 1e-4) for t in (W2, b1, b2)]
        la = torch.zeros(8, device=cuda)
        ca = torch.zeros(8, dtype=torch.int32, device=cuda)
        lg2 = torch.zeros(2, M, C, device=cuda)
        for step in range(3):
            cur = torch.tensor([step + 1], dtype=torch.int64, device=cuda)
            lg2[step & 1] = pool["lg"][:M, :C] * (1.0 + step)
            args = ([x0, Hh], [1 / 255.0, 1.0], [False, False], None, None, -1, M, [None, None],
                    [2, 1], [W2c, None], [Hh, None], 0.9, lg2, cur, -1, b2v, labels, 1.0 / M, la,
                    ca, 1, [W1, W2], [b1, b2], [m1, st[0]], [v1, st[3]], [st[1], st[2]],
                    [st[4], st[5]], 1e-3, None, 0.9, 0.999, 1e-8, 0.0, cur, 1.0, False, None,
                    None, 0)
            if impl == "hip":
                _ext().wgrad_grouped(*args, None, None, step & 1)
            else:
                ref.wgrad_grouped(*args, None, None, step & 1)
        out[impl] = (flats, W2, b1, b2)
    for fh, fr in zip(out["hip"][0], out["ref"][0]):
        _close(fh[pad:pad + N * K], fr[pad:pad + N * K], 2e-4, 1e-6, "padded P/M/V")
        assert torch.equal(fh[:pad], torch.full_like(fh[:pad], sent))
        assert torch.equal(fh[pad + N * K:], torch.full_like(fh[pad + N * K:], sent))
    for a, b in zip(out["hip"][1:], out["ref"][1:]):
        _close(a, b, 2e-4, 1e-6, "W2/b1/b2")


@pytest.mark.parametrize("M,N,C", list(itertools.product((1, 16, 100), (16, 20), (2, 10))))
def test_forward_logits_partial(cuda, M, N, C):
    """Logits of both parities on a zeroed buffer; the other parity buffer and everything past
    row M stay bit-unchanged."""
    g = torch.Generator().manual_seed(100 * M + 10 * N + C)
    data = torch.randint(0, 256, (ROWS, 784), generator=g, dtype=torch.uint8).to(cuda)
    idx = torch.randperm(ROWS, generator=g).to(torch.int32).to(cuda)
    labels = torch.randint(0, C, (ROWS,), generator=g, dtype=torch.uint8).to(cuda)
    W1 = (torch.randn(N, 784, generator=g) * 0.05).to(cuda)
    b1 = (torch.randn(N, generator=g) * 0.1).to(cuda)
    W2 = (torch.randn(C, N, generator=g) * 0.1).to(cuda)
    sent = 7.0
    for stepv in (3, 4):   # buffer 1, buffer 0
        out = {}
        for impl in ("hip", "ref"):
            A = torch.tensor([stepv], dtype=torch.int64, device=cuda)
            Bc = torch.zeros(1, dtype=torch.int64, device=cuda)
            H = torch.empty(M, N, device=cuda)
            w2c = torch.empty(C, N, device=cuda)
            flat = torch.full((2 * M * C + 16 * C,), sent, device=cuda)  # rows >= M: the tail
            lg2 = flat[:2 * M * C].view(2, M, C)
            lg2[stepv & 1] = 0.0
            xb = torch.zeros(M, 784, dtype=torch.uint8, device=cuda)
            yb = torch.zeros(M, dtype=torch.int32, device=cuda)
            args = (data, 1 / 255.0, idx, A, M, W1, b1, H, 0.9, 77, A, W2, w2c, lg2, xb, labels,
                    yb, Bc, A, 1)
            if impl == "hip":
                _ext().mlp_fwd_logits(*args, None)
            else:
                ref.mlp_fwd_logits(*args)
            out[impl] = (H, lg2, flat)
        h, r = out["hip"], out["ref"]
        _close(h[0], r[0], 1e-4, 1e-5, "H")
        _close(h[1][stepv & 1], r[1][stepv & 1], 1e-4, 1e-4, "logits")
        other = h[1][(stepv + 1) & 1]
        assert torch.equal(other, torch.full_like(other, sent))       # the other parity buffer
        tail = h[2][2 * M * C:]
        assert torch.equal(tail, torch.full_like(tail, sent))         # rows >= M


def test_small_trainer_graph_equals_eager(cuda):
    """4 eager steps against one 4-step graph at hidden=20, batch=5, in_dim=64 (criteria of
    test_graph_replay_equals_eager)."""
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, 256, (40, 64), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (40,), generator=g, dtype=torch.uint8)
    cfg = MLPConfig(in_dim=64, hidden=20, batch=5, seed=5)
    a = FusedMLPTrainer(cfg, x, y, device=cuda)
    b = FusedMLPTrainer(cfg, x, y, device=cuda)
    b.set_permutation(a.perm)
    assert a.enable_graphs(4)
    a.train_steps(4)
    b.train_steps(4)
    torch.cuda.synchronize()
    diff = (a.P - b.P).abs()
    off = diff > (1e-6 + 1e-4 * b.P.abs())
    assert float(off.float().mean()) < 1e-4, int(off.sum())
    assert float(diff.max()) < 20 * a.cfg.lr
    assert int(a.ctrA.item()) == 4
