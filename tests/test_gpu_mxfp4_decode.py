"""-m gpu: the MXFP4 weight stream of the Llama graph decoder (decode_weights="mxfp4").  The contract everything rests on: code * 2^e is
exactly a bf16 number, v_cvt_scalef32_pk_bf16_fp4 widens the codes under their block scale exactly, and the kernel runs the bf16 kernel's
MFMAs in the bf16 kernel's order, so vtgb_gemm_skinny_mxfp4 on the stream equals vtgb_gemm_skinny on the dequantised bf16 matrix BIT FOR
BIT -- fragments, deferred consumers, logits and ids included."""
import copy

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


def _dq(w):
    from videotgb_amd import ops
    return ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(w), dtype=w.dtype)


def _w_wide(N, K, dev, seed):
    """Gaussian weights whose 32-blocks are scaled by 2^-8 .. 2^8: the scale exponents span far more than a Gaussian's three."""
    g = torch.Generator(device=dev).manual_seed(seed)
    w = torch.randn(N, K // 32, 32, generator=g, device=dev)
    w = w * torch.ldexp(torch.ones((), device=dev), torch.randint(-8, 9, (N, K // 32, 1), generator=g, device=dev))
    return w.view(N, K).bfloat16()


# ------------------------------------------------------------------------------------------------------------- the pack kernel
@pytest.mark.parametrize("N,K", [(100, 128), (256, 64), (640, 448), (1000, 320), (4096, 4096)])
def test_pack_kernel_equals_the_host_recipe_bit_for_bit(dev, N, K):
    from videotgb_amd import ops
    w = _w_wide(N, K, dev, N + K)
    w[3].zero_()                                                    # an all-zero row
    w[5, 32:64].zero_()                                             # an all-zero block between others
    w[6, 40] = 3.0e4                                                # one large outlier: the rest of its block rounds to zero codes
    w[7, :8] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -4.0], device=dev).bfloat16() * 2.0 ** -5      # every midpoint, under e = -5
    w[7, 8:32].zero_()
    w[8, :32] = 2.0 ** -130                                         # bf16 subnormals: the lower clamp, zero codes
    w[9, :32] = 0.0
    w[9, 1] = 1.5 * 2.0 ** -121                                     # under the lower clamp with a non-zero code
    w[10, :32] = -7.75 * 2.0 ** 6                                   # saturation, negative
    w[11, 33] = 1.75 * 2.0 ** 127                                   # the largest exponent
    w[12, :32] = -0.0
    w[12, 0] = 1.0                                                  # negative zeros keep their sign bit
    sk = ops.SkinnyWeightMxfp4(w)
    codes, scales = ops.quantize_mxfp4_rows(w)
    assert sk.data.numel() * 32 == ops.SkinnyWeightFp8(w).data.numel() * 17
    assert torch.equal(sk.scales(), scales)
    assert torch.equal(sk.codes(), codes)
    assert (scales[3] == 127).all() and not codes[3].any() and scales[5, 1].item() == 127 and scales[8, 0].item() == 7 and scales[9, 0].item() == 7
    assert scales[11, 1].item() == 252 and codes[12, 1:16].eq(0x88).all()
    # rows beyond N: zero codes under the byte 127
    nt, nk = (N + 127) // 128, K // 64
    last = sk.data.view(nt, nk, 4096 + 256)[-1]
    rows_in = N - (nt - 1) * 128
    code_rows = last[:, :4096].reshape(nk, 4, 16, 4, 2, 2, 4).permute(1, 4, 2, 0, 5, 3, 6).reshape(128, -1)
    scale_rows = last[:, 4096:].reshape(nk, 4, 16, 2, 2).permute(1, 3, 2, 0, 4).reshape(128, -1)
    assert not code_rows[rows_in:].any() and (scale_rows[rows_in:] == 127).all()
    # the same quantisation on the CPU, and the two properties on these weights
    cc, sc = ops.quantize_mxfp4_rows(w.cpu())
    assert torch.equal(cc, codes.cpu()) and torch.equal(sc, scales.cpu())
    dq = ops.dequantize_mxfp4_rows(codes, scales, torch.float32)
    assert torch.isfinite(dq).all() and torch.equal(dq.bfloat16().float(), dq)
    # re-packing the dequantised matrix gives the same values (and the same stream but for the blocks whose every code is zero under a clamped scale)
    sk2 = ops.SkinnyWeightMxfp4(dq.bfloat16())
    assert torch.equal(sk2.codes(), codes)
    same = sk2.scales() == scales
    assert same.view(-1)[(codes.view(N, K // 32, 16) != 0).any(2).view(-1)].all() and same.float().mean().item() > 0.99


def test_non_finite_weights_and_bad_shapes_raise(dev):
    from videotgb_amd import ops
    w = _w_wide(128, 64, dev, 1)
    w[5, 5] = float("inf")
    with pytest.raises(ValueError):
        ops.SkinnyWeightMxfp4(w)
    with pytest.raises(NotImplementedError):
        ops.SkinnyWeightMxfp4(_w_wide(128, 64, dev, 1)[:, :32].contiguous())


# ------------------------------------------------------------------------------------------------------------- the GEMM
@pytest.mark.parametrize("M,N,K,S", [(5, 100, 128, 2), (77, 1000, 320, 3), (3, 640, 448, 1), (124, 4096, 4096, 0), (128, 256, 64, 0), (17, 200, 448, 3)])
def test_mxfp4_skinny_equals_the_exact_sum_over_the_dequantised_weights(dev, M, N, K, S):
    """Against an anchor that shares nothing with the kernels, with EQUALITY as the bound: x holds integers in [-3, 3] and the weights are
    Gaussian, whose block exponents e span at most four values, so every product x * dq is a multiple of u = 2^(emin - 1) no larger than
    3 * 6 * 2^emax and every partial sum of a row, in any order, is a multiple of u below 2^24 u (asserted): exact in fp32.  The reference
    is the fp64 matmul of the dequantised weights."""
    from videotgb_amd import ops
    g = torch.Generator(device=dev).manual_seed(M * 7 + N)
    x = torch.randint(-3, 4, (M, K), generator=g, device=dev).bfloat16()
    w = torch.randn(N, K, generator=g, device=dev).bfloat16()
    codes, scales = ops.quantize_mxfp4_rows(w)
    emin, emax = int(scales.min().item()) - 127, int(scales.max().item()) - 127
    assert emax - emin <= 3 and K * 18 * 2 ** (emax - emin + 1) < 2 ** 24
    dq = ops.dequantize_mxfp4_rows(codes, scales, torch.float64)
    ref = x.double() @ dq.t()
    assert torch.equal(ref.float().double(), ref)
    sk = ops.SkinnyWeightMxfp4(w)
    out32 = ops.gemm_skinny(x, sk, n_splits=S, out_dtype=torch.float32)
    assert torch.equal(out32, ref.float()), (out32 - ref.float()).abs().max().item()
    out = ops.gemm_skinny(x, sk, n_splits=S)
    assert out.dtype == torch.bfloat16 and torch.equal(out, out32.bfloat16())        # one rounding, of the reduced sum
    assert out32.abs().sum() > 0


def _fragments(x, w, S, bias=None):
    """(S the call used, its K-split fragments as the consumers read them) of a defer_reduce call with a workspace of its own."""
    from videotgb_amd import ops
    M, K = x.shape
    need = ops.gemm_skinny_workspace_bytes(M, w.N, K, S)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=x.device)
    _, S_used, ws_out = ops.gemm_skinny(x, w, n_splits=S, workspace=ws, defer_reduce=True, bias=bias)
    assert ws_out is ws
    return S_used, ws.view(torch.float32).clone()


@pytest.fixture(scope="module")
def ragged(dev):
    """N = 200: two tiles, the second partial; K = 448: 7 k-tiles, so every ring has steps past the split's end."""
    from videotgb_amd import ops
    N, K = 200, 448
    w = _w_wide(N, K, dev, 5)
    codes, scales = ops.quantize_mxfp4_rows(w)
    assert scales.unique().numel() >= 12
    g = torch.Generator(device=dev).manual_seed(9)
    bias = torch.randn(N, generator=g, device=dev)
    return N, K, ops.SkinnyWeightMxfp4(w), ops.SkinnyWeight(_dq(w)), bias


@pytest.mark.parametrize("M", [1, 16, 17, 32, 33, 64, 65, 128])
def test_mxfp4_skinny_equals_the_bf16_kernel_on_the_dequantised_weights(dev, ragged, M):
    """Every x-block specialisation (M <= 16, 32, 64, 128) and its first row past it, split and unsplit, fp32 and bf16 outputs, plain, with a
    bias and with the reduce left to the consumer (the fragments are equal)."""
    from videotgb_amd import ops
    N, K, sk4, sk16, bias = ragged
    g = torch.Generator(device=dev).manual_seed(M)
    x = torch.randn(M, K, generator=g, device=dev).bfloat16()
    for S in (0, 1, 3):
        for b in (None, bias):
            for od in (torch.float32, torch.bfloat16):
                a, r = ops.gemm_skinny(x, sk4, n_splits=S, out_dtype=od, bias=b), ops.gemm_skinny(x, sk16, n_splits=S, out_dtype=od, bias=b)
                assert torch.equal(a, r), (M, S, b is not None, od, (a.float() - r.float()).abs().max().item())
                assert torch.isfinite(a.float()).all() and a.float().abs().sum() > 0
        assert not torch.equal(ops.gemm_skinny(x, sk4, n_splits=S, bias=bias), ops.gemm_skinny(x, sk4, n_splits=S))
    for b in (None, bias):
        (s4, f4), (s16, f16) = _fragments(x, sk4, 3, b), _fragments(x, sk16, 3, b)
        assert s4 == s16 == 3 and torch.equal(f4, f16) and f4.abs().sum() > 0


def test_mxfp4_skinny_equals_the_bf16_kernel_at_a_production_shape(dev):
    from videotgb_amd import ops
    M, N, K = 124, 4096, 4096
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(M, K, generator=g, device=dev).bfloat16()
    w = _w_wide(N, K, dev, 3) * K ** -0.5
    sk4, sk16 = ops.SkinnyWeightMxfp4(w), ops.SkinnyWeight(_dq(w))
    bias = torch.randn(N, generator=g, device=dev)
    for od in (torch.float32, torch.bfloat16):
        assert torch.equal(ops.gemm_skinny(x, sk4, out_dtype=od), ops.gemm_skinny(x, sk16, out_dtype=od))
        assert torch.equal(ops.gemm_skinny(x, sk4, out_dtype=od, bias=bias), ops.gemm_skinny(x, sk16, out_dtype=od, bias=bias))
    (s4, f4), (s16, f16) = _fragments(x, sk4, 0), _fragments(x, sk16, 0)
    assert s4 == s16 > 1 and torch.equal(f4, f16)


# ------------------------------------------------------------------------------------------------------------- the decoder
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
H = 128


def _dequantised_copy(lm):
    ref = copy.deepcopy(lm)
    with torch.no_grad():
        mods = [getattr(part, n) for l in ref.model.layers for part in (l.self_attn, l.mlp) for n in PROJ if hasattr(part, n)] + [ref.lm_head]
        assert len(mods) == 7 * len(ref.model.layers) + 1
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


def _small_llama(dev, lora=False, **kw):
    """4 layers, hidden 128 = 2 heads of 64 over one K/V head, intermediate 256: every K a multiple of 64."""
    from videotgb_amd import llm
    lm = llm.build_llama("tiny", torch.bfloat16, dev, seed=2, hidden_size=H, intermediate_size=256, num_hidden_layers=4, num_attention_heads=2,
                         num_key_value_heads=1, **kw)
    with torch.no_grad():      # (N(0, 0.02) leaves near-uniform logits: a wider lm_head and embedding make the ids move)
        lm.lm_head.weight.mul_(40.0)
        lm.model.embed_tokens.weight.mul_(20.0)
        for n, p in lm.named_parameters():
            if n.endswith("proj.bias"):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))).to(p.device, p.dtype) * 0.2)
    if lora:
        import lora_refs
        from videotgb_amd import train
        train.apply_lora(lm)
        lora_refs.nonzero_lora_(lm, seed=5, std=0.3)
        lm.eval()
    return lm


def _pair(lm, **kw):
    from videotgb_amd.decode import GreedyDecoder
    dec4, dec16 = GreedyDecoder(lm, weights="mxfp4", **kw), GreedyDecoder(_dequantised_copy(lm), **kw)
    return dec4, dec16, _first_logits(dec4), _first_logits(dec16)


@pytest.fixture(scope="module")
def small(dev):
    lm = _small_llama(dev)
    yield (lm,) + _pair(lm)


def _emb(dev, B, P, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(B, P, H, generator=g, device=dev) * 0.5).bfloat16()


def _assert_streams_mxfp4(dec):
    st = next(reversed(dec.graphs.values()))
    assert "sk_ws" in st and st["graph"] is not None                                 # graph replay on the skinny path
    sw = dec._skinny_weights()
    assert all(type(w).__name__ == "SkinnyWeightMxfp4" for layer in sw[:-1] for w in layer) and type(sw[-1]).__name__ == "SkinnyWeightMxfp4"


@pytest.mark.parametrize("B", [1, 20])
@pytest.mark.parametrize("kind", ["unpadded", "padded", "sampled"])
def test_mxfp4_graph_decoder_equals_the_bf16_decoder_on_the_dequantised_model(dev, small, B, kind):
    lm, dec4, dec16, seen4, seen16 = small
    P, n_new = 9, 10
    emb = _emb(dev, B, P, B + len(kind))
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
    del seen4[:], seen16[:]
    out4 = dec4.generate(emb, n_new, **kw)
    out16 = dec16.generate(emb, n_new, **kw)
    _assert_streams_mxfp4(dec4)
    assert len(seen4) == len(seen16) == 1 and torch.equal(seen4[0], seen16[0]) and seen4[0].float().abs().sum() > 0
    assert out4.shape == (B, n_new) and torch.equal(out4, out16), (out4[:2].tolist(), out16[:2].tolist())
    assert torch.equal(dec4.generate(emb, n_new, **kw), out4)                                                                 # replay of the cached graph


@pytest.mark.parametrize("what", ["kv_fp8", "lora", "beams", "biases"])
def test_mxfp4_combines_with_the_decoders_other_modes(dev, what):
    """The fp8 K/V cache, unmerged LoRA adapters, beam search and projection biases, each on the mxfp4 stream: the ids (and, where a first token
    is picked from the prefill's logits, those logits) are the bf16 decoder's on the model that carries the dequantised weights."""
    B, P, n_new = 3, 9, 8
    lm = _small_llama(dev, lora=what == "lora", **(dict(attention_bias=True, mlp_bias=True) if what == "biases" else {}))
    dec4, dec16, seen4, seen16 = _pair(lm, **(dict(kv_cache="fp8") if what == "kv_fp8" else {}))
    if what == "biases":
        assert dec4.bias is not None
    if what == "lora":
        assert dec4.lora is not None
    emb = _emb(dev, B, P, 40 + len(what))
    am = torch.ones(B, P, dtype=torch.long)
    am[1, :2] = 0
    kw = dict(attention_mask=am)
    if what == "beams":
        kw.update(num_beams=3, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=None, pad_token_id=0)
    out4, out16 = dec4.generate(emb, n_new, **kw), dec16.generate(emb, n_new, **kw)
    st = next(reversed(dec4.graphs.values()))
    assert st["graph"] is not None and type(dec4._skinny_weights()[-1]).__name__ == "SkinnyWeightMxfp4"
    if what == "kv_fp8":
        assert st["attn"] == "split_fp8"
    if what == "beams":
        assert st["attn"] == "beam"
    assert len(seen4) == len(seen16) and all(torch.equal(a, b) for a, b in zip(seen4, seen16))
    assert out4.shape[0] == B and torch.equal(out4, out16), (out4.tolist(), out16.tolist())


def test_mxfp4_ids_differ_from_the_unquantised_models(dev, small):
    """(Otherwise the equalities above would hold for a decoder that ignored the switch.)"""
    from videotgb_amd.decode import GreedyDecoder
    lm, dec4, _, _, _ = small
    emb = _emb(dev, 16, 9, 11)
    assert not torch.equal(dec4.generate(emb, 12), GreedyDecoder(lm).generate(emb, 12))
    assert not torch.equal(dec4.head_w, lm.lm_head.weight)


# ------------------------------------------------------------------------------------------------------------- the public switch
def test_session_and_generate_on_an_mxfp4_model_and_requantisation_after_an_update(dev):
    """LSTP.from_cfg(..., decode_weights="mxfp4"): generate and a clip session decode through the same mxfp4 decoder (same ids), which are
    the ids of the default mode on a model whose LM carries the dequantised weights; after an in-place update of the LM's weights the next
    call decodes with re-quantised weights (decode.weights_key retires the decoder).  The tiny configuration with an LM of hidden size 64
    (the format's k-tile)."""
    from test_gpu_session import clip, questions
    from videotgb_amd import llm, models
    from videotgb_amd.synth import path_state_dict, synth_tensor, tiny_cfg
    cfg = tiny_cfg("instructblip")
    cfg.vit.image, cfg.llm_hidden = 56, 64
    sd = path_state_dict(cfg, seed=0)

    def model(lm, **kw):
        m = models.LSTP.from_cfg(cfg, dev, language_model=lm, compute_dtype="bf16", **kw)
        m.load_state_dict(sd, strict=False)
        return m.to(dev)
    lm = llm.build_llama("tiny", torch.bfloat16, dev, hidden_size=64, intermediate_size=128)
    lm.load_state_dict({k: synth_tensor("model.language_model." + k, tuple(v.shape)).to(dev) for k, v in lm.state_dict().items()}, strict=True)
    m4 = model(lm, decode_weights="mxfp4")
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
    got = run(m4)
    assert m4._decoder.weights == "mxfp4" and type(m4._decoder._skinny_weights()[-1]).__name__ == "SkinnyWeightMxfp4"
    want = run(model(_dequantised_copy(lm)))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    old = m4._decoder
    with torch.no_grad():
        for p in lm.model.layers.parameters():
            if p.dim() == 2:
                p.mul_(1.7)
    got2 = run(m4)
    assert m4._decoder is not old and m4._decoder.weights == "mxfp4"
    want2 = run(model(_dequantised_copy(lm)))
    assert all(torch.equal(a, b) for a, b in zip(got2, want2))
    assert any(not torch.equal(a, b) for a, b in zip(got, got2))
