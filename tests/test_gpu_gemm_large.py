"""-m gpu: vtgb_gemm's bf16 kernels at the sizes the models run them, against references (tests/gemm_ref.py; DESIGN.md has the table).

For bf16 vtgb_gemm dispatches to gemm_bf16_kernel (128 x 128 tile), to the persistent ping-pong kernel gemm_bf16_pp_kernel (K % 64 == 0, >= 200 tiles
of 256 x 256, pp_supported) or to gemm_bf16_large_kernel (the same size rule where pp_supported says no).  The shapes of test_gpu_kernels.py stay on
the first; these cases reach the other two, and EVERY case names the kernel it is meant to reach and asserts, through the profiler, that this kernel
and no other GEMM kernel ran: a change to the dispatch rule fails the tests instead of silently emptying them.

Exact cases: integer operands (A, W in {-2 .. 2}, integer bias and residual, |result| < 2**24), so that every fp32 epilogue must EQUAL the integer
result whatever the summation order; for the bf16 store operands in {-1, 0, 1} and K <= 192, so that |result| <= 256 is a bf16 number.
Bound cases: A ~ N(0, 1), W ~ 0.05 N(0, 1), bias and residual ~ N(0, 1) against gemm_ref.ref64 / gemm_ref.bound, element by element.
GELU is bound-only, and runs at K >= 640.  The bf16 epilogues' GELU is a fit of x Phi(x) with <= 2.6e-5 ABSOLUTE error (gelu_erf_fast, csrc/gemm_dev.h;
largest near x = +-3.06).  The bound's 2**-8 |ref| is used up by the bf16 rounding alone (half an ulp at the bottom of a binade), so the fit has to
fit into the accumulator term: 1.13 * 2e-6 * (s + 1) >= 2.6e-5 + 1.13 * 1.4e-7 * s needs s = sum |a||w| + |bias| >= 12.3.  At this distribution s is
0.032 K +- 0.04 sqrt(K): 10.2 +- 0.7 at K = 320 (short: measured there, 2 of 12 M elements at 1.003 x the bound),
20.4 +- 1 at K = 640.  The models run the GELU epilogue at K = 768 and 1408.

Every call runs through gemm_ref.run_gemm: operands are views into poisoned buffers (NaN behind A's and W's last rows and in their pad columns, a
bit pattern around out), with lda / ldw / ldo chosen per case."""
import re

import pytest
import torch

import gemm_ref as R
from gemm_ref import EPI_GELU, EPI_RESID_F32, EPI_STORE, EPI_STORE_F32

pytestmark = pytest.mark.gpu

PP, LARGE, SMALL, F32K = "gemm_bf16_pp_kernel", "gemm_bf16_large_kernel", "gemm_bf16_kernel<", "gemm_f32_kernel"
GEMM_KERNELS = (PP, LARGE, SMALL, F32K)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def gemm_kernels(names):
    return sorted({k for n in names for k in GEMM_KERNELS if k in n})


def pp_args(name):
    """Template arguments of a gemm_bf16_pp_kernel instantiation: <EPI, CONV, NWN, TAIL, PING, WF, LNF>."""
    m = re.search(r"gemm_bf16_pp_kernel<([^>]*)>", name)
    return [a.strip() for a in m.group(1).split(",")] if m else None


def is_true(arg):
    return arg in ("true", "1", "(bool)1")


def launch(kernel, *args, **kw):
    """run_gemm under the profiler: the declared kernel ran, and no other GEMM kernel did."""
    box = []
    names = R.kernels_run(lambda: box.append(R.run_gemm(*args, **kw)))
    assert gemm_kernels(names) == [kernel], f"meant to reach {kernel}, ran {[n for n in names if 'gemm' in n]}"
    if kernel == PP:      # the plain instantiation: ping-pong k-loop, no folded LayerNorm
        a = [pp_args(n) for n in names if PP in n]
        assert all(x is not None and not is_true(x[1]) and is_true(x[4]) and not is_true(x[6]) for x in a), names
    return box[0]


def int_operands(dev, M, N, K, amax, seed, dtype=torch.bfloat16):
    g = torch.Generator(device=dev).manual_seed(seed)
    A = torch.randint(-amax, amax + 1, (M, K), generator=g, device=dev).to(dtype)
    W = torch.randint(-amax, amax + 1, (N, K), generator=g, device=dev).to(dtype)
    bias = torch.randint(-8, 9, (N,), generator=g, device=dev).float()
    resid = torch.randint(-100, 101, (M, N), generator=g, device=dev).float()
    return A, W, bias, resid


def rand_operands(dev, M, N, K, seed, dtype=torch.bfloat16):
    g = torch.Generator(device=dev).manual_seed(seed)
    A = torch.randn(M, K, generator=g, device=dev).to(dtype)
    W = (torch.randn(N, K, generator=g, device=dev) * 0.05).to(dtype)
    return A, W, torch.randn(N, generator=g, device=dev), torch.randn(M, N, generator=g, device=dev)


def check_exact(tag, run):
    ref = R.ref64(run.A, run.W, run.bias, run.resid, run.epilogue)          # integers below 2**24: float64 IS the integer result
    assert ref.abs().max() < 2 ** 24 and (run.out.dtype == torch.float32 or ref.abs().max() <= 256)
    bad = (run.out.double() != ref).nonzero()
    assert bad.numel() == 0, f"{tag}: {bad.shape[0]} elements differ from the integer result, the first at (row, column) {bad[0].tolist()}: " \
                             f"{run.out[tuple(bad[0])].item()} for {ref[tuple(bad[0])].item()}"


def check_bound(tag, run):
    ex = R.excess(run)
    worst = ex.argmax()
    print(f"[{tag}] max |out - ref64| / bound = {ex.max().item():.3f} at (row, column) ({int(worst) // ex.shape[1]}, {int(worst) % ex.shape[1]}); "
          f"{int((ex > 1).sum())} of {ex.numel()} elements outside")
    assert ex.max() <= 1.0, tag


# ----------------------------------------------------------------------------- the edges
# (M, N, K) as functions of the CU count c: the persistent kernel's grid is min(tiles, c) workgroups that walk the tile list with stride grid, G = 8
# m-tiles per group.  `lay` is run_gemm's layout; `epis` the exact epilogues; "tiles" what test_edge asserts about the tile count.
def _m(tiles_m, last=256):
    return (tiles_m - 1) * 256 + last


EDGES = {
    # 1: fewer tiles than CUs, a grid that is no multiple of 8 (first_q's other branch), ONE n-tile whose last two 64-column wave groups are partly /
    #    wholly padding (N = 136), nk = 1
    "e1-fewer_tiles_than_cus-grid_not_x8-one_n_tile-nk1": dict(kernel=PP, M=lambda c: _m(203, 200), N=136, K=64, tiles=lambda t, c: 200 <= t < c and t % 8 != 0),
    # 2: grid = CU count, workgroups with one and with two tiles, last m-group shorter than G, last m-tile of 63 rows (three of four row-waves padding),
    #    last n-tile 136 wide
    "e2-grid_eq_cus-1_and_2_tiles-short_last_group-63_row_last_tile-nk2": dict(kernel=PP, M=lambda c: _m((c + 49) // 5, 63), N=1160, K=128,
                                                                            tiles=lambda t, c: c < t < 2 * c and (t // 5) % 8 != 0),
    # 3: three rounds, the last one partial; nk = 3 and nk = 5 against the three-slot ring
    "e3-three_rounds_partial_last-nk3": dict(kernel=PP, M=lambda c: _m((2 * c + 103) // 5, 250), N=1160, K=192, tiles=lambda t, c: 2 * c < t < 3 * c),
    "e3-three_rounds_partial_last-nk5": dict(kernel=PP, M=lambda c: _m((2 * c + 103) // 5, 250), N=1160, K=320, tiles=lambda t, c: 2 * c < t < 3 * c),
    # 4: more than 8 n-tiles (wide tile lists; G = 8 in gemm_bf16_large_kernel), N % 8 == 4
    "e4-nine_n_tiles[pp]": dict(kernel=PP, M=lambda c: _m(23, 256), N=2100, K=64, lay=dict(o_pad=4), tiles=lambda t, c: t == 207),
    "e4-nine_n_tiles[large]": dict(kernel=LARGE, M=lambda c: _m(23, 256), N=2100, K=64, lay=dict(w_pad=8), tiles=lambda t, c: t == 207),
    # 5 / 6: N % 8 == 2 on a bf16 store: with ldo % 8 == 0 the persistent kernel's "N % 8 store", with ldo = N the one-tile-per-workgroup kernel
    "e5-n_mod_8_is_2-bf16_store-ldo_x8[pp]": dict(kernel=PP, M=lambda c: _m(41, 77), N=1162, K=64, lay=dict(o_pad=6), epis=("store",)),
    "e6-n_mod_8_is_2-bf16_store-ldo_eq_n[large]": dict(kernel=LARGE, M=lambda c: _m(41, 77), N=1162, K=64, epis=("store",)),
    # 7: N % 4 != 0 on the fp32 epilogues (the early-residual path: the residual is loaded into the accumulators before the k-loop)
    "e7-n_mod_4_is_2-fp32_epilogues-early_residual[large]": dict(kernel=LARGE, M=lambda c: _m(41, 77), N=1162, K=128, epis=("store_f32", "resid_inplace", "resid_separate")),
    "e7-odd_n-all_epilogues[large]": dict(kernel=LARGE, M=lambda c: _m(41, 77), N=1161, K=128),
    # 8: ldw % 64 != 0 with K % 64 == 0: W a column slice of [N, K + 8]
    "e8-ldw_not_x64-bias_and_none[large]": dict(kernel=LARGE, M=lambda c: _m(41, 130), N=1160, K=128, lay=dict(w_off=8, w_pad=8), nobias=True),
    # 9: lda > K and ldw = K + 64: column slices the persistent kernel still takes
    "e9-lda_gt_k-ldw_k_plus_64-slices[pp]": dict(kernel=PP, M=lambda c: _m(41, 130), N=1160, K=128, lay=dict(a_off=8, a_pad=72, w_off=8, w_pad=64, o_pad=8)),
    # 10 / 11: the residual in place and separate, bias and none, on both kernels (every case here runs both residual forms; these two both bias forms)
    "e10_e11-resid_inplace_and_separate-bias_and_none[pp]": dict(kernel=PP, M=lambda c: _m(41, 256), N=1280, K=128, nobias=True),
    "e10_e11-resid_inplace_and_separate-bias_and_none[large]": dict(kernel=LARGE, M=lambda c: _m(41, 256), N=1280, K=128, lay=dict(w_pad=8), nobias=True),
    # 12: K % 64 != 0 at 200+ tiles stays on the 128 x 128 kernel
    "e12-k72_at_200_tiles-stays_small[small]": dict(kernel=SMALL, M=lambda c: 51_000, N=256, K=72, tiles=lambda t, c: t == 200),
}
EXACT_EPIS = ("store_f32", "resid_inplace", "resid_separate", "store")


def run_epi(kernel, name, A, W, bias, resid, lay):
    if name.startswith("resid"):
        return launch(kernel, A, W, bias, EPI_RESID_F32, resid, inplace=name == "resid_inplace", **lay)
    return launch(kernel, A, W, bias, {"store_f32": EPI_STORE_F32, "store": EPI_STORE, "gelu": EPI_GELU}[name], **lay)


@pytest.mark.parametrize("edge", list(EDGES), ids=list(EDGES))
def test_edge_exact_integers(dev, cus, edge):
    e = EDGES[edge]
    M, N, K, lay = e["M"](cus), e["N"], e["K"], e.get("lay", {})
    tiles = -(-M // 256) * -(-N // 256)
    assert tiles >= 200 and e.get("tiles", lambda t, c: True)(tiles, cus), f"{tiles} tiles on {cus} CUs: the shape no longer has the edge it is named for"
    for name in e.get("epis", EXACT_EPIS):
        if name == "store" and K > 192:
            continue                                               # (|result| <= 256 needs K <= 192; nk = 5 is covered by the fp32 epilogues)
        A, W, bias, resid = int_operands(dev, M, N, K, 1 if name == "store" else 2, seed=len(edge) + K)
        for b in (bias, None) if e.get("nobias") else (bias,):
            check_exact(f"{edge} {name} bias={b is not None}", run_epi(e["kernel"], name, A, W, b, resid, lay))


@pytest.mark.parametrize("edge", list(EDGES), ids=list(EDGES))
def test_edge_bound_random(dev, cus, edge):
    """The same launches on random operands: what integers cannot show (the bf16 rounding of the store, bias and residual that are no integers)."""
    e = EDGES[edge]
    M, N, K, lay = e["M"](cus), e["N"], e["K"], e.get("lay", {})
    A, W, bias, resid = rand_operands(dev, M, N, K, seed=len(edge) + K)
    for name in e.get("epis", EXACT_EPIS):
        for b in (bias, None) if e.get("nobias") else (bias,):
            check_bound(f"{edge} {name} bias={b is not None}", run_epi(e["kernel"], name, A, W, b, resid, lay))


@pytest.mark.parametrize("kernel,lay", [(PP, dict(o_pad=8)), (LARGE, dict(w_pad=8))], ids=["pp", "large"])
def test_e11_gelu_bias_and_none(dev, kernel, lay):
    """Edge 11's fourth epilogue (bound-only; K = 640: module docstring), 41 x 5 tiles, the last 136 wide."""
    A, W, bias, resid = rand_operands(dev, _m(41, 99), 1160, 640, seed=11)
    for b in (bias, None):
        check_bound(f"e11 gelu {kernel} bias={b is not None}", run_epi(kernel, "gelu", A, W, b, resid, lay))


@pytest.mark.parametrize("lay,K", [(dict(a_pad=4, w_off=4, w_pad=8, o_pad=3), 100), (dict(a_off=1, a_pad=3, w_pad=1, o_pad=1), 99)], ids=["vector_loads", "scalar_loads"])
def test_e13_fp32_kernel_padded_strides_exact_and_bound(dev, lay, K):
    """Edge 13: the fp32 kernel has the same public strides: padded lda / ldw / ldo with the sentinels, a few hundred rows, 16-byte rows and not."""
    M, N = 389, 203
    for name in EXACT_EPIS:
        A, W, bias, resid = int_operands(dev, M, N, K, 2, seed=K, dtype=torch.float32)
        for b in (bias, None):
            check_exact(f"e13 fp32 {name}", run_epi(F32K, name, A, W, b, resid, lay))
    # random integers / 64 times integers / 16: every product and partial sum is a multiple of 2**-10 below 2**7 -- still exact in fp32, in any order
    g = torch.Generator(device=dev).manual_seed(K)
    A = torch.randint(-64, 65, (M, K), generator=g, device=dev).float() / 64
    W = torch.randint(-16, 17, (N, K), generator=g, device=dev).float() / 16
    bias = torch.randint(-64, 65, (N,), generator=g, device=dev).float() / 32
    check_bound("e13 fp32 gelu", run_epi(F32K, "gelu", A, W, bias, None, lay))
    check_exact("e13 fp32 fractions", run_epi(F32K, "store_f32", A, W, bias, None, lay))


# ----------------------------------------------------------------------------- the depths the models use
DEPTHS = {
    "vit_g-K1408-34x6_tiles": (_m(34, 256), 1408, 1408),             # ViT-g's hidden size; 6 n-tiles, the last 128 wide
    "vit_g-K6144-34x6_tiles": (_m(34, 256), 1408, 6144),             # fc2
    "prefill-K4096-26x8_tiles": (_m(26, 100), 2048, 4096),           # the prefill's 26 m-tiles (the tile list csrc/gemm_pp.hip's comment names)
    "prefill-K11008-26x8_tiles": (_m(26, 100), 2048, 11008),         # down_proj
}


@pytest.mark.parametrize("shape", list(DEPTHS), ids=list(DEPTHS))
def test_bound_at_model_depths(dev, shape):
    M, N, K = DEPTHS[shape]
    A, W, bias, resid = rand_operands(dev, M, N, K, seed=K)
    for name in ("store", "gelu", "resid_inplace"):
        check_bound(f"{shape} {name}", run_epi(PP, name, A, W, bias, resid, {}))


def test_persistent_kernel_is_bit_reproducible(dev, cus):
    """Edge 3's shape (three rounds, every workgroup's tiles back to back through the LDS ring), twice: equal bits in every epilogue."""
    M, N, K = _m((2 * cus + 103) // 5, 250), 1160, 320
    A, W, bias, resid = rand_operands(dev, M, N, K, seed=3)
    for name in ("store", "gelu", "resid_inplace", "store_f32"):
        a, b = (run_epi(PP, name, A, W, bias, resid, {}).out for _ in range(2))
        bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(a.view(bits), b.view(bits)), name


# ----------------------------------------------------------------------------- the LayerNorm-folded instantiation, through vtgb_vit_forward
def test_vit_folded_layernorm_gemms_on_the_persistent_kernel(dev):
    """The folded GEMMs (GemmDesc::ln_*) are not reachable from vtgb_gemm: a small ViT (hidden 128, 2 heads of 64, mlp 512, 2 layers, 17 tokens) at 3 200
    frames has M = 54 400 rows, so every GEMM of a layer has >= 213 tiles and runs gemm_bf16_pp_kernel -- qkv / fc1 and projection / fc2 (all but the
    last) in the LNF instantiation -- and the patch embedding, 51 200 rows = exactly 200 m-tiles with segmented output / residual row maps, runs
    gemm_bf16_large_kernel.  Reference: the oracle's vit_embed / vit_layer in float64 on the device, and under torch.autocast(bfloat16); pass rule: the
    project's own for bf16 stages (test_gpu_stages.check_bf16_three_way), e_ref from the two oracle runs.  The unfolded table
    (fold_ln=False) passes the same rule on the same input."""
    from oracle import vtgb_oracle as O
    from test_gpu_stages import check_bf16_three_way, to_dev
    from videotgb_amd import ops
    from videotgb_amd.synth import VitCfg, synth_state_dict, vit_shapes
    cfg = VitCfg(hidden=128, layers=2, heads=2, mlp=512, image=56, patch=14)
    n = 3200
    assert cfg.tokens == 17 and n * (cfg.tokens - 1) == 200 * 256
    sd = to_dev(synth_state_dict(vit_shapes(cfg, ""), 0), dev)
    pix = torch.randn(n, 3, 56, 56, generator=torch.Generator(device=dev).manual_seed(4), device=dev)

    def embed_as_gemm(sd_, pix_):
        """oracle.vit_embed with the patch convolution (stride = kernel size) written as the GEMM it is: F.linear on the unfolded patches.  Under autocast
        it rounds the same operands to bf16 and the output once, as conv2d does, without the first-use build of a bf16 convolution kernel (seconds)."""
        w_ = sd_["embeddings.patch_embedding.weight"]
        g_ = cfg.image // cfg.patch
        cols = pix_.view(n, 3, g_, cfg.patch, g_, cfg.patch).permute(0, 2, 4, 1, 3, 5).reshape(n, g_ * g_, -1)
        x = torch.nn.functional.linear(cols, w_.reshape(cfg.hidden, -1), sd_["embeddings.patch_embedding.bias"])
        x = torch.cat([sd_["embeddings.class_embedding"].expand(n, 1, -1), x], dim=1)
        return x + sd_["embeddings.position_embedding"][:, : x.shape[1], :]

    def oracle(sd_, x):
        for i in range(cfg.layers):
            x = O.vit_layer(sd_, f"encoder.layers.{i}.", x, cfg.heads, cfg.eps)
        return torch.nn.functional.layer_norm(x, (cfg.hidden,), sd_["post_layernorm.weight"], sd_["post_layernorm.bias"], cfg.eps)

    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        x64 = O.vit_embed(sd64, "", pix.double())
        assert (embed_as_gemm(sd64, pix.double()) - x64).abs().max() <= 1e-12      # the restatement IS the oracle's embedding
        ref64 = oracle(sd64, x64).cpu()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ref16 = oracle(sd, embed_as_gemm(sd, pix)).float().cpu()
    for fold in (True, False):
        w = ops.VitWeights(sd, "", ops.BF16, cfg.heads, cfg.eps, fold_ln=fold)
        box = []
        names = R.kernels_run(lambda: box.append(ops.vit_forward(w, pix)[0]))
        pp = [pp_args(k) for k in names if PP in k]
        lnf = {int(a[0]) for a in pp if is_true(a[6])}
        assert any(re.search(LARGE + rf"<{EPI_RESID_F32}, false,", k) for k in names), \
            f"the patch embedding (200 m-tiles, row maps) is meant to reach {LARGE}<EPI_RESID_F32, false>: {names}"
        assert SMALL not in gemm_kernels(names), names
        if fold:      # consumers: qkv (EPI_STORE) and fc1 (EPI_GELU); producers: projection and fc2 (EPI_RESID_F32)
            assert lnf == {EPI_STORE, EPI_GELU, EPI_RESID_F32}, f"the LNF instantiations did not all run: {names}"
        else:
            assert not lnf and {int(a[0]) for a in pp} == {EPI_STORE, EPI_GELU, EPI_RESID_F32}, names
        check_bf16_three_way(f"small ViT, 3200 frames, fold_ln={fold}", box[0], ref64, ref16)
