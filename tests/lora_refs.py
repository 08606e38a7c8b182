"""Test infrastructure for the LoRA update (vtgb_llm_lora / ops.lora_update), in the manner of tests/llm_refs.py: the inputs, the fp64
reference and THE RULE a result is held to.  Nothing here comes from the code under test.

The update of one segment (col0, A [r, K], B [n, r], scaling) on y [rows, n_cols], for x [rows, K]:
    d = rnd((B (A x)) * scaling)        fp32 sums, fp32 product, one rounding to y's dtype
    y[:, col0 : col0 + n] = rnd(y[:, col0 : col0 + n] + d)
The fp64 reference is ``d_exact``.  Two nested fp32 sums (K terms, then r terms) and one fp32 product differ from it, in any summation
order and with or without fused multiply-adds, by at most
    e = (K + r + 3) * 2^-24 * (sum_i |B_ji| sum_k |A_ik x_k|) * |scaling|
(the standard bound for recursive / pairwise summation with unit roundoff 2^-24: K roundings at most on any path of the first sum, r on
the second, one for the product, two to spare for the second-order terms).  Rounding to the dtype and adding y are monotone maps, so

    THE RULE:  add(y, rnd(d_exact - e))  <=  got  <=  add(y, rnd(d_exact + e))      element-wise, in the dtype's own arithmetic
               (fp32: rnd is the identity on fp32 numbers, the second rounding is the add's), and
               columns outside every segment are bit-identical to y, and every value is finite.
"""
import torch

SEGMENTS = ((0, 32), (64, 40))      # (col0, n): columns 32..63 and 104..111 of a 112-column y are never written
N_COLS = 112


def make_case(dtype, K, r, rows, scaling, seed=0, segments=SEGMENTS, n_cols=N_COLS):
    """x [rows, K] and y [rows, n_cols] of ``dtype`` as column slices of wider buffers (row strides K + 8 and n_cols + 8), and one
    (col0, A, B, scaling) per segment: A ~ U(-1, 1) / sqrt(K) (peft's kaiming_uniform(a = sqrt(5))), B ~ N(0, 0.3)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * K + 3 * r + rows)
    x = torch.randn(rows, K + 8, generator=g).to(dtype)[:, :K]
    y = torch.randn(rows, n_cols + 8, generator=g).to(dtype)[:, :n_cols]
    segs = []
    for col0, n in segments:
        A = ((torch.rand(r, K, generator=g) * 2 - 1) / K ** 0.5).contiguous()
        B = (torch.randn(n, r, generator=g) * 0.3).contiguous()
        segs.append((col0, A, B, float(scaling)))
    return x, y, segs


def d_exact(x, A, B, scaling):
    """fp64: (B (A x)) * scaling, [rows, n]."""
    return ((x.double() @ A.double().T) @ B.double().T) * float(scaling)


def d_bound(x, A, B, scaling):
    """fp64 [rows, n]: the bound e of the module docstring."""
    K, r = A.shape[1], A.shape[0]
    mag = (x.double().abs() @ A.double().abs().T) @ B.double().abs().T
    return (K + r + 3) * 2.0 ** -24 * mag * abs(float(scaling))


def _add(y, d64):
    """add(y, rnd(d)) in y's own arithmetic: d rounded to the dtype (through fp32: monotone), the sum formed in fp32 and rounded once."""
    d = d64.float().to(y.dtype)
    return (y.float() + d.float()).to(y.dtype)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def verdict(x, y, segs, got):
    """None when ``got`` obeys the rule for the update of ``y`` (the values BEFORE the call), else what it breaks.  CPU tensors."""
    x, y, got = x.cpu(), y.cpu(), got.cpu()
    if got.shape != y.shape or got.dtype != y.dtype:
        return f"shape / dtype {tuple(got.shape)} {got.dtype}, expected {tuple(y.shape)} {y.dtype}"
    if not bool(torch.isfinite(got.float()).all()):
        return "non-finite values"
    touched = torch.zeros(y.shape[1], dtype=torch.bool)
    for col0, A, B, scaling in segs:
        n = B.shape[0]
        touched[col0: col0 + n] = True
        A, B = A.cpu(), B.cpu()
        d, e = d_exact(x, A, B, scaling), d_bound(x, A, B, scaling)
        y_s = y[:, col0: col0 + n]
        lo, hi, g = _add(y_s, d - e).double(), _add(y_s, d + e).double(), got[:, col0: col0 + n].double()
        bad = (g < lo) | (g > hi)
        if bool(bad.any()):
            m, j = [int(v) for v in bad.nonzero()[0]]
            return (f"{int(bad.sum())} of {bad.numel()} values of segment col0={col0} outside the rule; first at row {m} column {col0 + j}: "
                    f"got {g[m, j].item()!r}, allowed [{lo[m, j].item()!r}, {hi[m, j].item()!r}] (y {y_s[m, j].item()!r}, d {d[m, j].item()!r})")
    if not torch.equal(_bits(got[:, ~touched]), _bits(y[:, ~touched])):
        return "a column outside every segment changed"
    return None


def emulate(x, y, segs, order="sequential"):
    """The update in fp32 arithmetic on the host, with the two sums added sequentially or pairwise (two legitimate kernels)."""
    def total(p):      # fp32 sum over the last dimension
        if order == "sequential":      # (an explicit loop: torch.cumsum accumulates fp32 in fp64 on the host)
            acc = torch.zeros_like(p[..., 0])
            for k in range(p.shape[-1]):
                acc = acc + p[..., k]
            return acc
        while p.shape[-1] > 1:
            if p.shape[-1] % 2:
                p = torch.cat((p, torch.zeros_like(p[..., :1])), -1)
            p = p[..., 0::2] + p[..., 1::2]
        return p[..., 0]
    out = y.clone()
    xf = x.float()
    for col0, A, B, scaling in segs:
        t = total(xf[:, None, :] * A[None, :, :])                       # [rows, r]
        u = total(t[:, None, :] * B[None, :, :])                        # [rows, n]
        d = (u * torch.tensor(scaling, dtype=torch.float32)).to(y.dtype)
        n = B.shape[0]
        out[:, col0: col0 + n] = (y[:, col0: col0 + n].float() + d.float()).to(y.dtype)
    return out


# ---- adapters for the decoder tests
def nonzero_lora_(lm, seed=0, std=0.3):
    """lora_B ~ N(0, std) on every adapter of ``lm`` (apply_lora leaves B = 0, which changes nothing), in place."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if "lora_B" in n:
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device, p.dtype))
    return lm
