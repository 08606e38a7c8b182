"""TEST INFRASTRUCTURE (not collected by pytest, not product).  Torch-only references, acceptance rules and input sets for the language-model
step kernels of csrc/llm.hip, shared by tests/test_llm_refs.py (CPU: the rules against an fp32 emulation of the kernels and against mutants)
and tests/test_gpu_llm_kernels.py (the kernels themselves).  Everything here works on whatever device its inputs live on.

References are fp64 with the roundings the kernels state (llm.hip's header: where modeling_llama / modeling_t5 round to the activation
dtype).  A rule raises AssertionError and otherwise returns the measured off-centre share."""
import torch

BF16, F32 = torch.bfloat16, torch.float32
CAP = 5e-3                 # share of elements of one call that may differ from the centre value (bf16)
FLOOR = 2.0 ** -22         # activations: four fp32 ulps of 1 in the cancelling 1 + tanh / 1 + erf / 1 + exp term, times |g| / 2
# The two GELU kinds are held to CAP on g >= GELU_CAP_FROM only: below, fp32 cancellation in 1 + tanh / 1 + erf moves several percent of
# the bf16 results by design.  The figure comes from the CPU measurement in tests/test_llm_refs.py, never from what a kernel produced.
GELU_CAP_FROM = -1.0
# SiLU is held to CAP on g >= -88: below -88.7 expf(-g) overflows in fp32 and the kernel's g / (1 + inf) is -0 where fp64 still has a tiny
# normal number (g = -90: -7e-38) -- the floor accepts that element, and it is no rounding flip, so it is not counted as one (one such edge
# value alone is 12 % of a 1 x 8 call).
SILU_CAP_FROM = -88.0
EDGES = (0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, -90.0, 100.0, -100.0, -104.0, -5.1875, -5.4375)
KINDS = {0: "silu", 1: "gelu_new", 2: "relu", 3: "gelu"}


# ------------------------------------------------------------------------------------------------------------------------ number formats
def same_bits(a, b):
    """bit for bit (torch.equal holds -0 == +0 and never NaN == NaN)"""
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def rnd(t64, dtype):
    """fp64 -> dtype in ONE rounding (torch goes through fp32 on the way to bf16: a value that lands exactly on a bf16 tie in fp32 without
    having been one is first moved one fp32 step back towards where it was)"""
    f = t64.float()
    if dtype == F32:
        return f
    tie = (f.view(torch.int32) & 0xFFFF) == 0x8000
    back = torch.where(f.double() < t64, torch.full_like(f, float("inf")), torch.full_like(f, float("-inf")))
    f = torch.where(tie & (f.double() != t64), torch.nextafter(f, back), f)
    return f.bfloat16()


def bf16_neighbours(t):
    """the next lower and the next higher bf16 value of each element (+-0 are one value; the largest finite value's upper neighbour is inf)"""
    assert t.dtype == BF16
    b = t.contiguous().view(torch.int16).to(torch.int32)
    key = torch.where(b >= 0, b, -(b & 0x7FFF))                       # monotone in the value
    def back(k):
        k = k.clamp(-0x7F80, 0x7F80)
        bits = torch.where(k >= 0, k, (-k) | 0x8000)
        return torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(BF16).view(t.shape)
    return back(key - 1), back(key + 1)


# ----------------------------------------------------------------------------------------------------------------------------- RMSNorm
def rmsnorm_ref(x, delta, w, eps, dtype):
    """-> x_new, n, h.  x_new = x + delta in dtype (torch's own add: one rounding), rs = (mean(x_new^2) + eps)^-1/2 in fp64,
    n = round(x_new rs), h = round(w n)."""
    x_new = x if delta is None else x + delta
    xd = x_new.double()
    e = torch.tensor(eps, dtype=F32).double().item()                   # (the entry takes eps as a float)
    rs = (xd.square().mean(-1, keepdim=True) + e).rsqrt()
    n = rnd(xd * rs, dtype)
    return x_new, n, rnd(w.double() * n.double(), dtype)


def check_rmsnorm(h, x_after, x, delta, w, eps, dtype, cap=CAP):
    """x afterwards is x_new bit for bit.  bf16: every h[i] is bf16(w[i] n') with n' = n[i] or one of its two bf16 neighbours -- a 1-ulp fp32
    difference in rs can flip the rounding of n and nothing else (w n' is exact in fp32: one rounding) -- and at most `cap` of the
    elements differ from the centre value.  fp32: |h - ref| <= 1e-5 |ref| (rs: ~1e-6 after a 4096-term fp32 sum; two roundings of 2^-24)."""
    x_new, n, ref = rmsnorm_ref(x, delta, w, eps, dtype)
    assert h.dtype == dtype and h.shape == ref.shape
    assert same_bits(x_after, x_new), "x after the call is not x + delta in one rounding"
    assert torch.isfinite(h).all()
    if dtype == F32:
        err = (h.double() - ref.double()).abs() - 1e-5 * ref.double().abs()
        assert (err <= 0).all(), f"fp32 rmsnorm: {int((err > 0).sum())} elements outside 1e-5 |ref|, worst excess {err.max().item():.3e}"
        return 0.0
    lo, hi = bf16_neighbours(n)
    wf = w.float()
    cands = [(wf * c.float()).bfloat16() for c in (n, lo, hi)]
    ok = (h == cands[0]) | (h == cands[1]) | (h == cands[2])
    assert ok.all(), f"bf16 rmsnorm: {int((~ok).sum())} of {ok.numel()} elements are none of the three candidates"
    share = (h != cands[0]).double().mean().item()
    assert share <= cap, f"bf16 rmsnorm: {share:.3e} of the elements off the centre value (cap {cap})"
    return share


def rmsnorm_inputs(rows, H, dtype, seed, device="cpu"):
    """-> x, delta, w.  Rows at scales 1e-3, 1e3, 1 in turn (another row's rs cannot pass); the last row of two or more is all zeros in x
    and delta; w has mixed signs."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([(1e-3, 1e3, 1.0)[r % 3] for r in range(rows)])[:, None]
    x = torch.randn(rows, H, generator=g) * scale
    delta = torch.randn(rows, H, generator=g) * scale * 0.5
    w = torch.randn(H, generator=g)
    if rows > 1:
        x[-1].zero_()
        delta[-1].zero_()
    return x.to(dtype).to(device), delta.to(dtype).to(device), w.to(dtype).to(device)


# ------------------------------------------------------------------------------------------------------------------------- activations
def act_f64(kind, g):
    """the four formulas of llm.hip's comment on vtgb_llm_gated_act, in fp64"""
    g = g.double()
    if kind == 0:
        return g / (1.0 + torch.exp(-g))
    if kind == 1:
        return 0.5 * g * (1.0 + torch.tanh(0.7978845608028654 * (g + 0.044715 * g * g * g)))
    if kind == 2:
        return torch.clamp_min(g, 0.0)
    if kind == 3:
        return 0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752440))
    raise ValueError(kind)


def act_ref(kind, g, u, dtype):
    """-> s, ref.  s = round(f64(g)); ref = round(s u), or s itself when ungated (u None)."""
    s = rnd(act_f64(kind, g), dtype)
    return s, (s if u is None else rnd(s.double() * u.double(), dtype))


def check_act(got, kind, g, u, dtype, cap=CAP, cap_from=None):
    """ReLU: equal to the reference (+-0 compare equal: fmaxf leaves the sign of a zero open).  Other kinds, bf16: got is bf16(s' u) with
    s' = s or one of its two neighbours, or |got - f64(g) u| <= FLOOR max(1, |g|) max(1, |u|) (which also covers exp(-g) overflowing to
    inf where fp64 gives a tiny number); at most `cap` of the elements differ from the centre value -- SiLU over g >= SILU_CAP_FROM (every
    element whose expf(-g) is finite), the GELU kinds over g >= GELU_CAP_FROM.  fp32: |got - ref| <= 1e-5 |ref| + the same floor (fp32 results differ from a correctly rounded fp64 one in
    the last place as a matter of course: no share is taken)."""
    s, ref = act_ref(kind, g, u, dtype)
    assert got.dtype == dtype and got.shape == ref.shape
    if kind == 2:
        assert torch.equal(got, ref), f"relu: {int((got != ref).sum())} elements differ"
        return 0.0
    gd = g.double()
    ud = torch.ones_like(gd) if u is None else u.double()
    floor = FLOOR * gd.abs().clamp_min(1.0) * ud.abs().clamp_min(1.0)
    exact = act_f64(kind, g) * ud
    gap = (got.double() - exact).abs()
    if dtype == F32:
        err = (got.double() - ref.double()).abs() - (1e-5 * ref.double().abs() + floor)
        assert (err <= 0).all(), f"fp32 {KINDS[kind]}: {int((~(err <= 0)).sum())} elements outside 1e-5 |ref| + floor"
        return 0.0
    lo, hi = bf16_neighbours(s)
    uf = torch.ones_like(s, dtype=F32) if u is None else u.float()
    cands = [(c.float() * uf).bfloat16() for c in (s, lo, hi)]
    ok = (got == cands[0]) | (got == cands[1]) | (got == cands[2]) | (gap <= floor)
    assert ok.all(), f"bf16 {KINDS[kind]}: {int((~ok).sum())} of {ok.numel()} elements are neither a candidate nor within the floor"
    region = g.double() >= ((SILU_CAP_FROM if kind == 0 else GELU_CAP_FROM) if cap_from is None else cap_from)
    if not region.any():
        return 0.0
    share = (got != cands[0])[region].double().mean().item()
    assert share <= cap, f"bf16 {KINDS[kind]}: {share:.3e} of the elements off the centre value (cap {cap})"
    return share


def act_inputs(rows, I, dtype, seed, device="cpu"):
    """-> g, u [rows, I].  g = 3 randn with the edge values spread over the rows and both ends of a row (a single element keeps its random
    draw); u = randn."""
    gen = torch.Generator().manual_seed(seed)
    g = 3.0 * torch.randn(rows, I, generator=gen)
    u = torch.randn(rows, I, generator=gen)
    for k, e in enumerate(EDGES if rows * I > 1 else ()):
        r = k % rows if k % 2 == 0 else rows - 1 - (k % rows)
        c = (k // 2) % I if k % 2 == 0 else I - 1 - ((k // 2) % I)
        g[r, c] = e
    return g.to(dtype).to(device), u.to(dtype).to(device)


# --------------------------------------------------------------------------------------------------------------------------- fragments
def make_fragments(cols, S, M, seed, device="cpu"):
    """-> part [cols / 128, S, M, 128] fp32, delta [M, cols] bf16.  The layout gemm_skinny.hip states under "fragments": column i of row
    r, split sp, sits at part[((i >> 7) S + sp) M + r][i & 127].  delta = the fp32 sum over sp in ascending order (sequential adds),
    rounded once to bf16 -- what the consumers of the fragments must see."""
    assert cols % 128 == 0
    gen = torch.Generator().manual_seed(seed)
    part = torch.randn(cols // 128, S, M, 128, generator=gen).to(device)
    acc = torch.zeros(cols // 128, M, 128, device=device)
    for sp in range(S):
        acc = acc + part[:, sp]
    return part, acc.permute(1, 0, 2).reshape(M, cols).bfloat16()


# ------------------------------------------------------------------------------------------------------ the input sets of both test files
# (rows, H): every arm of vtgb_llm_rmsnorm's dispatch -- the vector kernels at H = 256 NV (16 / sizeof T), the scalar one elsewhere
RMS_SHAPES = {BF16: [(3, 4096), (130, 4096), (3, 2048), (2, 100), (4, 257), (1, 1), (2, 8192), (3, 1024)],
              F32: [(3, 4096), (3, 2048), (2, 100), (4, 257), (3, 1024)]}
RMS_EPS = (1e-6, 1e-5)
# (rows, I) of vtgb_llm_silu_mul: (2, 2056) leaves the second block partial, (65536, 8) has rows > 65535, (300, 3501) exceeds 4096 x 256
# elements (the grid-stride loop)
SILU_SHAPES = [(3, 11008), (1, 8), (2, 2056), (3, 100), (5, 7), (2, 11), (65536, 8), (300, 3501)]
ACT_SHAPES = [(3, 100), (1, 1), (300, 3501)]
