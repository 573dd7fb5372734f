"""The MNIST step's backward with 112-row LDS images (runs on an MI355X).

The compiled pair of the MNIST step (``wgrad_grouped`` with both head modes, C <= 10) stages and
multiplies 112 rows instead of 128 when the batch has at most 112: the staging items that held
only padding rows and the K-loop steps that multiplied only zeros are gone. The chain assignment
and the order of the non-zero additions are those of the 128-row images, so every output must
equal the 128-row path bit for bit. That path is the same compiled pair with the switch
``_C.wgrad_short_images(False)``, and in gradient mode also the generic kernel, which a launch
takes when its labels are int64. (In Adam mode the generic kernel's epilogue is compiled apart
from the pair's and rounds differently in the last bit, with or without this change.)

This file carries the name the issue gave it. The replicated logits accumulators it was also
meant to test were measured and not kept (``docs/perf.md``, "Logits accumulators: one copy per
group of n-tiles"), and their tests left with them.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 300
SENT = 7.0


def _ext():
    from arena_amd.ops import _ext
    return _ext.load()


@pytest.fixture(scope="module")
def pool(cuda):
    """Random source material, generated once and sliced per case (never written)."""
    g = torch.Generator().manual_seed(4321)
    p = {
        "data": {K: torch.randint(0, 256, (ROWS, K), generator=g, dtype=torch.uint8).to(cuda)
                 for K in (64, 100, 784)},
        "labels": torch.randint(0, 16, (ROWS,), generator=g).to(cuda),
        "idx": torch.randperm(ROWS, generator=g).to(torch.int32).to(cuda),
        "H": torch.relu(torch.randn(128, 36, generator=g)).to(cuda),
        "W2c": (torch.randn(16, 36, generator=g) * 0.1).to(cuda),
        "lg": torch.randn(128, 16, generator=g).to(cuda),
        "b2": torch.randn(16, generator=g).to(cuda),
        "bstate": torch.randn(4, 36, generator=g).to(cuda),
        "W1": (torch.randn(36, 784, generator=g) * 0.01).to(cuda),
        "b1": (torch.randn(36, generator=g) * 0.1).to(cuda),
        "W2": (torch.randn(16, 36, generator=g) * 0.05).to(cuda),
    }
    p["H"][p["H"] < 0.3] = 0.0
    return p


def _backward(pool, cuda, M, C, N, K, mode, cur, parity, gather, pair, nobias=()):
    """One backward launch (hidden layer: head mode 2, output layer: head mode 1). pair: the
    launch qualifies for the compiled pair when C <= 10 (a device learning rate, labels of the
    pair's dtype); else it runs the generic kernel (no device learning rate, int64 labels).
    nobias: problems without a bias. Returns every buffer the launch may write."""
    hs = cur - 1
    data = pool["data"][K]
    lab_all = pool["labels"] % C
    Hh = pool["H"][:M, :N].contiguous()
    W2c = pool["W2c"][:C, :N].contiguous()
    b2v = pool["b2"][:C].contiguous()
    if gather:
        x0, labels, idx = data, lab_all.to(torch.uint8), pool["idx"]
    else:
        x0, labels, idx = data[:M].contiguous(), lab_all[:M].to(torch.int32), None
    if not pair:
        labels = labels.to(torch.int64)
    curt = torch.tensor([cur], dtype=torch.int64, device=cuda)
    lg2 = torch.full((2, M, C), SENT, device=cuda)
    lg2[hs & 1] = pool["lg"][:M, :C]
    W1 = pool["W1"][:N, :K].clone()
    W2 = pool["W2"][:C, :N].clone()
    bs = pool["bstate"]
    b1, b2 = pool["b1"][:N].clone(), b2v.clone()
    st = [torch.full_like(W1, 1e-3), torch.full_like(W2, 1e-3), bs[0, :N] * 1e-3,
          bs[1, :C] * 1e-3, torch.full_like(W1, 1e-4), torch.full_like(W2, 1e-4),
          bs[2, :N].abs() * 1e-4 + 1e-6, bs[3, :C].abs() * 1e-4 + 1e-6]
    st = [t.clone() for t in st]
    outB, mB, vB = [b1, b2], [st[2], st[3]], [st[6], st[7]]
    for i in nobias:
        outB[i] = mB[i] = vB[i] = None
    la = torch.zeros(8, device=cuda)
    ca = torch.zeros(8, dtype=torch.int32, device=cuda)
    la[(hs + 1) & 7] = SENT
    lr_t = torch.full((1,), 1e-3, device=cuda) if pair else None
    _ext().wgrad_grouped(
        [x0, Hh], [1 / 255.0, 1.0], [gather, False], idx, curt if gather else None, -1, M,
        [None, None], [2, 1], [W2c, None], [Hh, None], 0.9, lg2, curt, -1, b2v, labels, 1.0 / M,
        la, ca, mode, [W1, W2], outB, [st[0], st[1]], [st[4], st[5]], mB, vB, 1e-3, lr_t, 0.9,
        0.999, 1e-8, 0.0, curt, 1.0, False, None, None, 0, None, None, parity)
    return [W1, W2, b1, b2] + st + [la, ca, lg2]


# counter 6 -> step 5 (parity 1), counter 7 -> step 6 (parity 0); -1 reads it from the counter
@pytest.mark.parametrize("cur,parity", [(6, -1), (6, 1), (7, 0)])
@pytest.mark.parametrize("mode", [0, 1])
def test_short_images_equal_128_row_path(cuda, pool, mode, cur, parity):
    """Every M x C x N x K of the issue (M 112 / 113 straddle the switch to 112 rows) and M 60 /
    65, which straddle the switch between the K-loop's single chain and its four: the threshold
    stays at 64 rows whatever the image height. Published batch and dataset gather, the logits
    buffer named at launch and by the counter, problems with and without a bias. C = 16 runs
    the generic kernel on every side."""
    cases = itertools.product((1, 5, 60, 65, 100, 112, 113, 128), (2, 10, 16), (16, 20, 36),
                              (64, 100, 784))
    for i, (M, C, N, K) in enumerate(cases):
        gather = bool((i + mode + cur) & 1)
        nobias = ((), (), (0,), (1,))[(i // 2) % 4]
        what = f"mode{mode} M{M} C{C} N{N} K{K} cur{cur} par{parity} g{int(gather)} nobias{nobias}"
        a = _backward(pool, cuda, M, C, N, K, mode, cur, parity, gather, True, nobias)
        _ext().wgrad_short_images(False)
        try:
            b = _backward(pool, cuda, M, C, N, K, mode, cur, parity, gather, True, nobias)
        finally:
            _ext().wgrad_short_images(True)
        for k, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"{what}: output {k} differs from the 128-row pair"
        if mode == 0:
            g = _backward(pool, cuda, M, C, N, K, mode, cur, parity, gather, False, nobias)
            for k, (x, y) in enumerate(zip(a, g)):
                assert torch.equal(x, y), f"{what}: output {k} differs from the generic kernel"
        hs = cur - 1
        assert float(a[-1][(hs + 1) & 1].abs().sum()) == 0.0, what    # next logits buffer zeroed
        assert float(a[-3][(hs + 1) & 7]) == 0.0, what                # next metric slot zeroed
