"""The operands of the MFMA tile kernels as ops/_terms.py packs them, bit for bit against the
formulas written out here (CPU only)."""
import numpy as np
import torch

from orange3_spark_amd.ops import fm, glm, linear_predict, mlp

THREE_TERMS = 1.0 + 2.0 ** -10 + 2.0 ** -20     # hi = 1, mid = 2^-10, lo = 2^-20
BIG_BIAS = 345.678901234                        # fp32(b) is off by ~1e-5: lo carries it


def _terms(Wp: torch.Tensor) -> torch.Tensor:
    """bf16 [3, ...]: successive round-to-nearest-even bf16 of the fp32 remainder."""
    hi = Wp.to(torch.bfloat16)
    r1 = Wp - hi.to(torch.float32)
    mid = r1.to(torch.bfloat16)
    r2 = r1 - mid.to(torch.float32)
    return torch.stack([hi, mid, r2.to(torch.bfloat16)])


def _padded(W: torch.Tensor, rows: int, D: int) -> torch.Tensor:
    out = torch.zeros(rows, D, dtype=torch.float32)
    out[:W.shape[0], :W.shape[1]] = W.to(torch.float32)
    return out


def _two_floats(x64: np.ndarray):
    hi = x64.astype(np.float32)
    return hi, (x64 - hi.astype(np.float64)).astype(np.float32)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a: torch.Tensor, b: torch.Tensor):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(_bits(a), _bits(b))


def _weights(rows: int, cols: int, seed: int) -> torch.Tensor:
    W = torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    W[0, 0] = THREE_TERMS
    return W


def test_three_terms_and_two_floats_are_needed():
    t = _terms(torch.tensor([THREE_TERMS], dtype=torch.float32)).to(torch.float64)
    assert t[0, 0] == 1.0 and t[1, 0] == 2.0 ** -10 and t[2, 0] == 2.0 ** -20
    hi, lo = _two_floats(np.array([BIG_BIAS]))
    assert lo[0] != 0.0 and float(hi[0]) + float(lo[0]) == BIG_BIAS


def test_softmax_operands():
    K, d = 5, 40
    W, b = _weights(K, d, 1).float(), torch.tensor([BIG_BIAS, -1.0, 0.5, 2.0, 3.0])
    D, Wsp, bp = glm.softmax_operands(W, b, torch.device("cpu"))
    assert D == 64 and Wsp.is_contiguous()
    _same(Wsp, _terms(_padded(W, 32, 64)))
    assert Wsp[2, 0, 0] != 0
    want = torch.zeros(32)
    want[:K] = b
    _same(bp, want)


def test_fm_operands():
    d, F = 40, 7
    V, w, w0 = _weights(d, F, 2), _weights(d, 1, 3)[:, 0], BIG_BIAS
    D, Wsp, sv, w0p, V64 = fm._pack(V, w, w0, torch.device("cpu"))
    assert D == 64 and Wsp.is_contiguous() and w0p.is_contiguous()
    Wp = torch.zeros(32, 64, dtype=torch.float32)
    Wp[:F, :d] = V.float().T
    Wp[F, :d] = w.float()
    _same(Wsp, _terms(Wp))
    assert Wsp[2, 0, 0] != 0
    s = torch.zeros(64)
    s[:d] = (V.float().double() ** 2).sum(1).float()
    _same(sv, s)
    hi, lo = _two_floats(np.array([w0]))
    _same(w0p, torch.from_numpy(np.concatenate([hi, lo])))
    assert w0p[1] != 0
    assert torch.equal(V64, V.float().double())


def test_linear_predict_pack():
    K, d = 40, 70                      # two blocks of 32 outputs, D = 96
    W = _weights(K, d, 4)
    b = np.linspace(-3.0, 3.0, K)
    b[0], b[1], b[2] = BIG_BIAS, -np.inf, 1e300
    p = linear_predict.pack(W.numpy(), b)
    assert p.wsp.shape == (2, 3, 32, 96) and p.wsp.dtype == np.int16 and p.wsp.flags.c_contiguous
    want = _terms(_padded(W, 64, 96)).view(3, 2, 32, 96).permute(1, 0, 2, 3)
    _same(torch.from_numpy(p.wsp).view(torch.bfloat16), want.contiguous())
    assert p.wsp[0, 2, 0, 0] != 0
    bp = np.zeros(64)
    bp[:K] = b
    with np.errstate(over="ignore", invalid="ignore"):
        hi, lo = _two_floats(bp)
    lo[~np.isfinite(hi)] = 0.0         # -inf and the overflow to +inf carry no lo
    assert p.bias_hi.shape == p.bias_lo.shape == (2, 32)
    _same(torch.from_numpy(p.bias_hi), torch.from_numpy(hi.reshape(2, 32)))
    _same(torch.from_numpy(p.bias_lo), torch.from_numpy(lo.reshape(2, 32)))
    assert p.bias_lo[0, 0] != 0 and p.bias_lo[0, 1] == 0 and p.bias_lo[0, 2] == 0


def test_mlp_pack():
    d, H, K = 70, 40, 5                # NH = 2, D = 96
    W1, W2 = _weights(d, H, 5), _weights(H, K, 6)
    b1, b2 = torch.linspace(-2, 2, H, dtype=torch.float64), torch.linspace(-1, 1, K, dtype=torch.float64)
    b1[0] = b2[0] = BIG_BIAS
    p = mlp.pack(W1, b1, W2, b2)
    assert (p.d, p.H, p.K) == (d, H, K) and p.W1sp.is_contiguous() and p.W2p.is_contiguous()
    _same(p.W1sp, _terms(_padded(W1.T, 64, 96)))
    assert p.W1sp[2, 0, 0] != 0
    t3 = _terms(_padded(W2, 64, 32))                      # [t, unit, class]
    want = torch.zeros(2, 2, 2, 3, 64, 8, dtype=torch.bfloat16)
    r = torch.arange(32)
    for j in range(2):
        for s in range(2):
            for h in range(2):
                for e in range(8):
                    k = 16 * s + 8 * (e >> 2) + 4 * h + (e & 3)
                    want[0, j, s, :, 32 * h + r, e] = t3[:, 32 * j + k, r]
                    want[1, j, s, :, 32 * h + r, e] = t3[:, 32 * j + r, k]
    _same(p.W2p, want)
    bias = np.zeros(64 * 2 + 64, dtype=np.float32)
    b1h, b1l = _two_floats(b1.numpy())
    b2h, b2l = _two_floats(b2.numpy())
    bias[:H], bias[64:64 + H] = b1h, b1l
    bias[128:128 + 32] = -np.inf
    bias[128:128 + K], bias[160:160 + K] = b2h, b2l
    _same(p.bias, torch.from_numpy(bias))
    assert p.bias[64] != 0 and p.bias[160] != 0
