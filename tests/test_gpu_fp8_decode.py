"""-m gpu: the fp8 weight stream of the Llama graph decoder (decode_weights="fp8").  The contract everything rests on: q * scale is exactly a
bf16 number and the fp8 kernel runs the bf16 kernel's MFMAs in the bf16 kernel's order, so vtgb_gemm_skinny_fp8 on the codes equals
vtgb_gemm_skinny on the dequantised bf16 matrix BIT FOR BIT -- fragments, deferred consumers, logits and ids included."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _w(N, K, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).bfloat16()


def _dq(w):
    from videotgb_amd import ops
    return ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(w))


# ------------------------------------------------------------------------------------------------------------- the pack kernel
@pytest.mark.parametrize("N,K", [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (32000, 4096), (100, 128), (1000, 320), (640, 448), (256, 64)])
def test_pack_kernel_equals_the_host_recipe_bit_for_bit(dev, N, K):
    from videotgb_amd import ops
    w = _w(N, K, dev, N + K)
    if N == 100:      # the recipe's corners on the device: a zero row, an amax of exactly 448 * 2^k, a row of subnormal codes and ties
        w[3].zero_()
        w[5, 7] = 448.0 * 2.0 ** -3
        w[6] = (torch.arange(K, device=dev) % 9).to(torch.bfloat16) * 2.0 ** -10
        w[6, 0] = 448.0
        w[7, :4] = torch.tensor([17.0, 19.0, -17.0, 448.0], device=dev).bfloat16()
    sk = ops.SkinnyWeightFp8(w)
    q, scale = ops.quantize_fp8_rows(w)
    assert sk.data.numel() * 2 == ops.SkinnyWeight(w).data.numel()
    assert torch.equal(sk.scale, scale)
    assert torch.equal(sk.codes().view(torch.uint8), q.view(torch.uint8))
    # rows beyond N: zero codes
    nt, nk = (N + 127) // 128, K // 64
    tail = sk.data.view(nt, nk, 128, 64)[-1, :, N - (nt - 1) * 128:]
    assert tail.numel() == 0 or not tail.any()
    # the same quantisation on the CPU
    qc, sc = ops.quantize_fp8_rows(w.cpu())
    assert torch.equal(qc.view(torch.uint8), q.cpu().view(torch.uint8)) and torch.equal(sc, scale.cpu())


def test_non_finite_weights_raise(dev):
    from videotgb_amd import ops
    w = _w(128, 64, dev, 1)
    w[5, 5] = float("inf")
    with pytest.raises(ValueError):
        ops.SkinnyWeightFp8(w)


# ------------------------------------------------------------------------------------------------------------- the GEMM
@pytest.mark.parametrize("M,N,K,S", [(124, 12288, 4096, 0), (124, 4096, 4096, 0), (124, 22016, 4096, 0), (124, 4096, 11008, 0), (124, 32000, 4096, 0),
                                     (1, 4096, 4096, 0), (32, 4096, 11008, 8), (128, 256, 64, 0), (5, 100, 128, 2), (77, 1000, 320, 3), (124, 4096, 4096, 17), (3, 640, 448, 1)])
def test_fp8_skinny_matches_fp32_matmul_of_the_dequantised_weights(dev, M, N, K, S):
    """The shapes and the bound of tests/test_gpu_skinny.py::test_skinny_matches_fp32_matmul, against an anchor that shares nothing with
    the kernels: x . dq^T in torch fp32 (exact products, fp32 accumulation -- only the summation order differs)."""
    from videotgb_amd import ops
    g = torch.Generator(device=dev).manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g, device=dev).bfloat16()
    w = (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).bfloat16()
    q, scale = ops.quantize_fp8_rows(w)
    ref = x.float() @ ops.dequantize_fp8_rows(q, scale, torch.float32).t()
    sk = ops.SkinnyWeightFp8(w)
    out32 = ops.gemm_skinny(x, sk, n_splits=S, out_dtype=torch.float32)
    err, bound = (out32 - ref).abs().max().item(), 2e-5 * ref.abs().max().item() * max(1.0, (K / 4096) ** 0.5)
    print(f"M={M} N={N} K={K} S={S}: max|err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    out = ops.gemm_skinny(x, sk, n_splits=S)
    assert out.dtype == torch.bfloat16 and torch.equal(out, out32.bfloat16())        # one rounding, of the reduced sum
    assert torch.equal(ops.gemm_skinny(x, sk, n_splits=S), out)                        # deterministic
    assert torch.equal(ops.gemm_skinny(x, sk, n_splits=S, out_dtype=torch.float32), out32)


@pytest.mark.parametrize("M", [1, 5, 16, 17, 32, 48, 64, 65, 124, 128])
def test_fp8_skinny_equals_the_bf16_kernel_on_the_dequantised_weights(dev, M):
    """Every x-block specialisation (M <= 16, 32, 64, 128), split and unsplit, fp32 and bf16 outputs, full and ragged N."""
    from videotgb_amd import ops
    g = torch.Generator(device=dev).manual_seed(M)
    for N, K, splits in ((4096, 4096, (0, 1, 3)), (1000, 320, (0, 1, 2, 5)), (22016, 4096, (0,)), (4096, 11008, (0, 2))):
        x = torch.randn(M, K, generator=g, device=dev).bfloat16()
        w = _w(N, K, dev, M + N)
        sk8, sk16 = ops.SkinnyWeightFp8(w), ops.SkinnyWeight(_dq(w))
        for S in splits:
            for od in (torch.float32, torch.bfloat16):
                a, b = ops.gemm_skinny(x, sk8, n_splits=S, out_dtype=od), ops.gemm_skinny(x, sk16, n_splits=S, out_dtype=od)
                assert torch.equal(a, b), (M, N, K, S, od, (a.float() - b.float()).abs().max().item())
        assert a.abs().sum() > 0


@pytest.mark.parametrize("M", [1, 124])
def test_fp8_deferred_split_consumers_equal_the_two_launch_form_bit_for_bit(dev, M):
    """tests/test_gpu_skinny.py's deferred-split test on the fp8 stream: the fragments are scaled before they leave the kernel, so
    vtgb_llm_rmsnorm_parts / vtgb_llm_rope_cache_parts consume them untouched -- and give what the bf16 kernel gives on dq."""
    from videotgb_amd import _lib as L, ops
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(M)
    H, nq, hd, tmax = 4096, 32, 128, 64
    for K in (4096, 11008):                                          # o (S = 4) and down (S = 7)
        a = torch.randn(M, K, generator=g, device=dev).bfloat16()
        wb = _w(H, K, dev, K)
        w, w16 = ops.SkinnyWeightFp8(wb), ops.SkinnyWeight(_dq(wb))
        gam = torch.randn(H, generator=g, device=dev).bfloat16()
        x0 = torch.randn(M, H, generator=g, device=dev).bfloat16()
        delta = ops.gemm_skinny(a, w)
        assert torch.equal(delta, ops.gemm_skinny(a, w16))
        xa, ha = x0.clone(), torch.empty_like(x0)
        L.check(lib.vtgb_llm_rmsnorm(L.BF16, xa.data_ptr(), delta.data_ptr(), gam.data_ptr(), ha.data_ptr(), M, H, 1e-6, st))
        out, S, ws = ops.gemm_skinny(a, w, defer_reduce=True)
        assert S > 1 and S == ops.gemm_skinny(a, w16, defer_reduce=True)[1]
        xb, hb = x0.clone(), torch.empty_like(x0)
        L.check(lib.vtgb_llm_rmsnorm_parts(L.BF16, xb.data_ptr(), ws.data_ptr(), S, gam.data_ptr(), hb.data_ptr(), M, H, 1e-6, st))
        assert torch.equal(xa, xb) and torch.equal(ha, hb), K
    a = torch.randn(M, H, generator=g, device=dev).bfloat16()
    wb = _w(3 * H, H, dev, 3)
    cos, sin = torch.randn(tmax, hd, generator=g, device=dev).bfloat16(), torch.randn(tmax, hd, generator=g, device=dev).bfloat16()
    pos = torch.tensor([5], device=dev)
    res = []
    for w, deferred in ((ops.SkinnyWeightFp8(wb), False), (ops.SkinnyWeightFp8(wb), True), (ops.SkinnyWeight(_dq(wb)), True)):
        q = torch.zeros(M, nq * hd, dtype=torch.bfloat16, device=dev)
        kc = torch.zeros(M, nq, tmax, hd, dtype=torch.bfloat16, device=dev)
        vc = torch.zeros_like(kc)
        if deferred:
            _, S, ws = ops.gemm_skinny(a, w, defer_reduce=True)
            assert S > 1
            L.check(lib.vtgb_llm_rope_cache_parts(L.BF16, ws.data_ptr(), S, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                  pos.data_ptr(), M, nq, nq, hd, tmax, st))
        else:
            qkv = ops.gemm_skinny(a, w)
            L.check(lib.vtgb_llm_rope_cache(L.BF16, qkv.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                            pos.data_ptr(), M, nq, nq, hd, tmax, st))
        res.append((q, kc, vc))
    for other in res[1:]:
        for t0, t1 in zip(res[0], other):
            assert torch.equal(t0, t1) and t0.abs().sum() > 0


# ------------------------------------------------------------------------------------------------------------- the decoder
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _dequantised_copy(lm):
    ref = copy.deepcopy(lm)
    with torch.no_grad():
        mods = [getattr(part, n) for l in ref.model.layers for part in (l.self_attn, l.mlp) for n in PROJ if hasattr(part, n)] + [ref.lm_head]
        for m in mods:
            m.weight.copy_(_dq(m.weight))
    return ref


def _first_logits(dec):
    """Records the logits the first token is picked from (the prefill's: ``_pick`` is called with the host step 0)."""
    seen = []
    pick = dec._pick

    def recorder(st, logits, step):
        if not isinstance(step, torch.Tensor):
            seen.append(logits.clone())
        return pick(st, logits, step)
    dec._pick = recorder
    return seen


@pytest.fixture(scope="module")
def vicuna4(dev):
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=2, num_hidden_layers=4)
    with torch.no_grad():      # (N(0, 0.02) leaves near-uniform logits: a wider lm_head and embedding make the ids move)
        lm.lm_head.weight.mul_(4.0)
        lm.model.embed_tokens.weight.mul_(20.0)
    dec8, dec16 = GreedyDecoder(lm, weights="fp8"), GreedyDecoder(_dequantised_copy(lm))
    yield lm, dec8, dec16, _first_logits(dec8), _first_logits(dec16)
    del lm, dec8, dec16
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [1, 124])
@pytest.mark.parametrize("kind", ["unpadded", "padded", "sampled"])
def test_fp8_graph_decoder_equals_the_bf16_decoder_on_the_dequantised_model(dev, vicuna4, B, kind):
    lm, dec8, dec16, seen8, seen16 = vicuna4
    P, n_new = 9, 10
    g = torch.Generator(device=dev).manual_seed(B + len(kind))
    emb = (torch.randn(B, P, 4096, generator=g, device=dev) * 0.5).bfloat16()
    kw = {}
    if kind == "padded":
        am = torch.ones(B, P, dtype=torch.long)
        am[0, :3] = 0                                              # left pads
        if B > 1:
            am[1, -2:] = 0                                         # right pads
            am[2, 4] = 0
        kw["attention_mask"] = am
    if kind == "sampled":
        kw.update(do_sample=True, temperature=0.7, top_k=50, top_p=0.9,
                  sample_noise=torch.rand(n_new, B, generator=torch.Generator().manual_seed(7)))
    del seen8[:], seen16[:]
    out8 = dec8.generate(emb, n_new, **kw)
    out16 = dec16.generate(emb, n_new, **kw)
    assert "sk_ws" in next(reversed(dec8.graphs.values())) and next(reversed(dec8.graphs.values()))["graph"] is not None      # graph replay on the skinny path
    assert isinstance(dec8._skinny_weights()[0][0], type(dec8._skinny_weights()[-1])) and type(dec8._skinny_weights()[-1]).__name__ == "SkinnyWeightFp8"
    assert len(seen8) == len(seen16) == 1 and torch.equal(seen8[0], seen16[0]) and seen8[0].float().abs().sum() > 0
    assert out8.shape == (B, n_new) and torch.equal(out8, out16), (out8[:2].tolist(), out16[:2].tolist())
    assert torch.equal(dec8.generate(emb, n_new, **kw), out8)                                                                 # replay of the cached graph


def test_fp8_ids_differ_from_the_unquantised_models(dev, vicuna4):
    """(Otherwise the equalities above would hold for a decoder that ignored the switch.)"""
    from videotgb_amd.decode import GreedyDecoder
    lm, dec8, _, _, _ = vicuna4
    g = torch.Generator(device=dev).manual_seed(11)
    emb = (torch.randn(16, 9, 4096, generator=g, device=dev) * 0.5).bfloat16()
    plain = GreedyDecoder(lm)
    assert not torch.equal(dec8.generate(emb, 12), plain.generate(emb, 12))
    assert not torch.equal(dec8.head_w, lm.lm_head.weight)


# ------------------------------------------------------------------------------------------------------------- the public switch
def test_session_and_generate_on_an_fp8_model_and_requantisation_after_an_update(dev, tiny_sd):
    """LSTP.from_cfg(..., decode_weights="fp8"): generate and a clip session decode through the same fp8 decoder (same ids), which are the
    ids of the default mode on a model whose LM carries the dequantised weights; after an in-place update of the LM's weights the next
    call decodes with re-quantised weights (decode.weights_key retires the decoder)."""
    from test_gpu_session import clip, questions
    from videotgb_amd import llm, models
    from videotgb_amd.synth import synth_tensor
    cfg, sd = tiny_sd["instructblip"]

    def model(lm, **kw):
        m = models.LSTP.from_cfg(cfg, dev, language_model=lm, compute_dtype="bf16", **kw)
        m.load_state_dict(sd, strict=False)
        return m.to(dev)
    lm = llm.build_llama("tiny", torch.bfloat16, dev)
    lm.load_state_dict({k: synth_tensor("model.language_model." + k, tuple(v.shape)).to(dev) for k, v in lm.state_dict().items()}, strict=True)
    m8 = model(lm, decode_weights="fp8")
    T, nframe = 12, 4
    frames, flow_frames = clip(cfg, dev, T)
    qs = questions("instructblip", cfg, dev, [(5, 7, 4), (9, 3, 6)], T)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=8, min_new_tokens=8)

    def run(m):
        sess = m.clip_session(frames, flow_frames)
        outs = []
        for te, se, noise in qs:
            ids, cand = m.generate(frames, flow_frames, nframe, te, se, noise=noise, **kw)
            ids_s, cand_s = sess.generate(nframe, te, se, noise=noise, **kw)
            assert torch.equal(ids, ids_s) and torch.equal(cand, cand_s)
            outs.append(ids)
        return outs
    got = run(m8)
    assert m8._decoder.weights == "fp8"
    want = run(model(_dequantised_copy(lm)))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    old = m8._decoder
    with torch.no_grad():
        for p in lm.model.layers.parameters():
            if p.dim() == 2:
                p.mul_(1.7)
    got2 = run(m8)
    assert m8._decoder is not old and m8._decoder.weights == "fp8"
    want2 = run(model(_dequantised_copy(lm)))
    assert all(torch.equal(a, b) for a, b in zip(got2, want2))
    assert any(not torch.equal(a, b) for a, b in zip(got, got2))
