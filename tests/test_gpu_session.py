"""-m gpu: clip sessions (videotgb_amd.session) -- many questions about one clip, RAFT and the TGB trunk once, each candidate frame
through ViT-g at most once.  A session promises BIT-identical answers: every comparison here is torch.equal against the path it replaces
(TemporalEncoder.forward for the split TGB, model.generate question by question for the session)."""
import random

import pytest
import torch

from test_gpu_stages import to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class BE(dict):
    __getattr__ = dict.__getitem__


# ---------------------------------------------------------------------------------------------------------------------------- TGB split
@pytest.mark.parametrize("size", ["tiny", "base"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["multi_modal", "fusion", "vision"])
@pytest.mark.parametrize("B", [1, 3])
def test_trunk_resume_equals_forward(dev, tiny_sd, size, dtype, mode, B):
    """vtgb_tgb_trunk on the clip + vtgb_tgb_resume on B question rows == TemporalEncoder.forward on the clip repeated B times, bit for bit
    (logits and sequence output), padded question masks; the tiny TGB (2 layers, fusion_layer 1) and BERT-base at T = 96."""
    from videotgb_amd import models
    from videotgb_amd.synth import TgbCfg, synth_state_dict, tgb_shapes
    if size == "tiny":
        cfg, psd = tiny_sd["instructblip"]
        cfg = cfg.tgb
        sd = {k[len("temporal_encoder."):]: v for k, v in psd.items() if k.startswith("temporal_encoder.")}
        T = 12
    else:
        cfg = TgbCfg()
        sd = synth_state_dict(tgb_shapes(cfg, ""), 0)
        T = 96
    te = models.TemporalEncoder(cfg, dtype)
    te.load_state_dict(to_dev(sd, dev), strict=False)
    te.to(dev)
    g = torch.Generator(device=dev).manual_seed(21)
    of = torch.rand(1, T, 2, 224, 224, generator=g, device=dev) * 2 - 1
    of_mask = torch.ones(1, T + 2, dtype=torch.long, device=dev)
    if size == "tiny":
        of_mask[0, -4:] = 0                                          # a clip shorter than the flow tensor
    nt = 9
    ids = torch.randint(3, cfg.vocab, (B, nt), generator=g, device=dev)
    mask = torch.ones(B, nt, dtype=torch.long, device=dev)
    mask[0, -2:] = 0
    if B > 1:
        mask[2, -5:] = 0
    seq_ref, logits_ref = te(encoder_embeds=of.expand(B, -1, -1, -1, -1).contiguous(), attention_mask=of_mask.expand(B, -1).contiguous(),
                             encoder_hidden_states=ids, encoder_attention_mask=mask, mode=mode)
    tr = te.trunk(encoder_embeds=of, attention_mask=of_mask, mode=mode)
    assert tr.H.shape == (T + 2, cfg.hidden) and tr.Hb.dtype == (torch.bfloat16 if dtype == "bf16" else torch.float32)
    seq, logits = te.resume(tr, encoder_hidden_states=ids, encoder_attention_mask=mask)
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()
    assert torch.equal(logits, logits_ref), (logits - logits_ref).abs().max().item()
    assert torch.equal(seq, seq_ref), (seq - seq_ref).abs().max().item()
    # the trunk is reusable: a second resume on different rows of the same clip
    seq2, logits2 = te.resume(tr, encoder_hidden_states=ids[:1], encoder_attention_mask=mask[:1])
    assert torch.equal(logits2[0], logits_ref[0]) and torch.equal(seq2[0], seq_ref[0])


# ----------------------------------------------------------------------------------------------------------------------- the session
def _tiny_t5(dev, d_model):
    from transformers import T5Config, T5ForConditionalGeneration
    torch.manual_seed(0)
    cfg = T5Config(vocab_size=120, d_model=d_model, d_kv=16, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=2, feed_forward_proj="gated-gelu",
                   tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, architectures=["T5ForConditionalGeneration"])
    lm = T5ForConditionalGeneration(cfg).eval()
    for p in lm.parameters():
        p.data.normal_(0, 0.3)
    return lm.to(dev)


def build(arch, tiny_sd, dev, dtype):
    """LSTP + tiny Llama / LSTP_blip2 + tiny T5 at the fixtures' tiny path, seeded weights, RAFT loaded."""
    from videotgb_amd import llm, models
    from videotgb_amd.synth import synth_tensor
    cfg, sd = tiny_sd[arch]
    if arch == "instructblip":
        lm = llm.build_llama("tiny", torch.float32, dev)
        lm.load_state_dict({k: synth_tensor("model.language_model." + k, tuple(v.shape)).to(dev) for k, v in lm.state_dict().items()}, strict=True)
        cls = models.LSTP
    else:
        lm = _tiny_t5(dev, cfg.llm_hidden)
        cls = models.LSTP_blip2
    m = cls(cfg, dev, language_model=lm, compute_dtype=dtype)
    m.load_state_dict(sd, strict=False)
    m.to(dev)
    return m, cfg, sd


def clip(cfg, dev, T=12, N=8, image=56, seed=30):
    g = torch.Generator(device=dev).manual_seed(seed)
    frames = torch.randn(N, 3, image, image, generator=g, device=dev)
    flow_frames = torch.rand(1, T, 3, 224, 224, generator=g, device=dev) * 255
    return frames, flow_frames


def questions(arch, cfg, dev, lengths, T, seed=31, lm_vocab=120):
    """One (text_encoding, sampler_text_encoding, noise) per entry of ``lengths`` = (sampler, prompt, qformer) token counts."""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for ls, lp, lq in lengths:
        sids = torch.randint(3, cfg.tgb.vocab, (1, ls), generator=g, device=dev)
        pids = torch.randint(3, lm_vocab, (1, lp), generator=g, device=dev)
        te = BE(input_ids=pids, attention_mask=torch.ones_like(pids))
        if arch == "instructblip":
            qids = torch.randint(3, cfg.qformer.vocab, (1, lq), generator=g, device=dev)
            te["qformer_input_ids"], te["qformer_attention_mask"] = qids, torch.ones_like(qids)
        se = BE(input_ids=sids, attention_mask=torch.ones_like(sids))
        noise = -torch.empty(2, 2, T, device=dev).exponential_(generator=g).log()
        out.append((te, se, noise))
    return out


STAGES = ("of", "tgb_logits", "frame_idx", "sampled", "prefix", "inputs_embeds")


def assert_same(got, ref, what):
    ids, cand, st = got
    rids, rcand, rst = ref
    assert torch.equal(ids, rids), f"{what}: ids {ids.tolist()} vs {rids.tolist()}"
    assert torch.equal(cand, rcand), f"{what}: cand_index {cand.tolist()} vs {rcand.tolist()}"
    for k in STAGES:
        assert st[k].shape == rst[k].shape and torch.equal(st[k], rst[k]), f"{what}: stage {k} differs"


LENGTHS = [(5, 7, 4), (9, 3, 6), (7, 11, 5), (3, 5, 8)]


@pytest.mark.parametrize("arch", ["instructblip", "blip2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fast_decode", ["auto", False])
def test_session_equals_generate_per_question(dev, tiny_sd, arch, dtype, fast_decode):
    m, cfg, _ = build(arch, tiny_sd, dev, dtype)
    T, nframe = 12, 4
    frames, flow_frames = clip(cfg, dev, T)
    qs = questions(arch, cfg, dev, LENGTHS, T)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=6, return_stages=True, fast_decode=fast_decode)
    refs = [m.generate(frames, flow_frames, nframe, te, se, noise=noise, **kw) for te, se, noise in qs]
    sess = m.clip_session(frames, flow_frames)
    for i, (te, se, noise) in enumerate(qs):
        assert_same(sess.generate(nframe, te, se, noise=noise, **kw), refs[i], f"{arch} {dtype} question {i}")
    order = list(range(len(qs)))
    random.Random(5).shuffle(order)
    sess2 = m.clip_session(frames, flow_frames)
    for i in order:
        te, se, noise = qs[i]
        assert_same(sess2.generate(nframe, te, se, noise=noise, **kw), refs[i], f"{arch} {dtype} shuffled question {i}")


@pytest.mark.parametrize("arch", ["instructblip", "blip2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batched_questions_equal_single_questions(dev, tiny_sd, arch, dtype):
    """Three equal-length questions in ONE sess.generate call: every pre-decode stage row equals the single-question call, bit for bit,
    and so do the greedy ids (graph decoder; min_new_tokens = max_new_tokens keeps the rows the same length)."""
    m, cfg, _ = build(arch, tiny_sd, dev, dtype)
    T, nframe, B = 12, 4, 3
    frames, flow_frames = clip(cfg, dev, T)
    qs = questions(arch, cfg, dev, [(6, 5, 4)] * B, T, seed=33)
    te = BE({k: torch.cat([q[0][k] for q in qs]) for k in qs[0][0]})
    se = BE({k: torch.cat([q[1][k] for q in qs]) for k in qs[0][1]})
    noise = torch.cat([torch.stack([q[2][:, 0] for q in qs], 1), torch.stack([q[2][:, 1] for q in qs], 1)], 1)     # [2, 2B, T]
    kw = dict(do_sample=False, temperature=None, max_new_tokens=6, min_new_tokens=6, return_stages=True, fast_decode="auto")
    sess = m.clip_session(frames, flow_frames)
    ids, cand, st = sess.generate(nframe, te, se, noise=noise, **kw)
    assert st["frame_idx"].shape == (B, nframe) and st["prefix"].shape[0] == B
    for i, (tei, sei, ni) in enumerate(qs):
        ids1, cand1, st1 = sess.generate(nframe, tei, sei, noise=ni, **kw)
        assert torch.equal(st["of"][i], st1["of"][0])
        assert torch.equal(st["tgb_logits"][i], st1["tgb_logits"][0]), i
        assert torch.equal(st["frame_idx"][i], st1["frame_idx"][0]), i
        assert torch.equal(st["sampled"][i * nframe:(i + 1) * nframe], st1["sampled"]), i
        assert torch.equal(st["prefix"][i], st1["prefix"][0]), i
        assert torch.equal(st["inputs_embeds"][i], st1["inputs_embeds"][0]), i
        assert torch.equal(ids[i], ids1[0]), (i, ids[i].tolist(), ids1[0].tolist())
    assert torch.equal(cand, st["frame_idx"][-1])


@pytest.mark.parametrize("arch", ["instructblip", "blip2"])
def test_session_work_done(dev, tiny_sd, arch):
    """Across 6 questions RAFT runs once and ViT-g encodes each selected frame exactly once (<= N frames in all)."""
    m, cfg, _ = build(arch, tiny_sd, dev, "bf16")
    T, N, nframe = 12, 8, 4
    frames, flow_frames = clip(cfg, dev, T, N)
    counts = {"raft": 0, "vit_frames": 0}
    raft_fwd, vit_fwd = m.of_extractor.forward_clips, m.model.vision_model.forward

    def raft_counted(x, *a, **k):
        counts["raft"] += 1
        return raft_fwd(x, *a, **k)

    def vit_counted(pixel_values=None, *a, **k):
        counts["vit_frames"] += pixel_values.shape[0]
        return vit_fwd(pixel_values, *a, **k)

    m.of_extractor.forward_clips = raft_counted
    m.model.vision_model.forward = vit_counted
    try:
        qs = questions(arch, cfg, dev, [(4 + i, 5, 3 + i % 3) for i in range(6)], T, seed=34)
        sess = m.clip_session(frames, flow_frames)
        seen = set()
        for te, se, noise in qs:
            _, _, st = sess.generate(nframe, te, se, noise=noise, do_sample=False, temperature=None, max_new_tokens=3, return_stages=True)
            seen |= set(st["frame_idx"].flatten().tolist())
            assert counts["vit_frames"] == len(seen)
        assert counts["raft"] == 1
        assert counts["vit_frames"] == len(seen) <= N
        assert sess.raft_calls == 1 and sess.vit_frames_encoded == len(seen)
        sess.prefetch()
        assert counts["vit_frames"] == N and counts["raft"] == 1
    finally:
        del m.of_extractor.forward_clips, m.model.vision_model.forward


def test_session_full_size(dev):
    """Vicuna-7B geometry (4-layer LM), EVA-ViT-g, the BERT-base TGB at T = 96, RAFT in its default mode (f16c8): three questions, each
    bit-equal to its own generate call."""
    from videotgb_amd import llm, models, synth
    cfg = synth.full_cfg("instructblip")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=4)
    m = models.LSTP(cfg, dev, language_model=lm, compute_dtype="bf16")
    m.load_state_dict(synth.path_state_dict(cfg, seed=0, with_raft=True), strict=False)
    m.to(dev)
    assert m.of_extractor.code == 3                                     # VTGB_F16C8
    T, N, nframe = 96, 32, 8
    frames, flow_frames = clip(cfg, dev, T, N, image=224, seed=40)
    qs = questions("instructblip", cfg, dev, [(12, 20, 12), (8, 14, 9), (15, 24, 14)], T, seed=41, lm_vocab=32000)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=8, return_stages=True)
    sess = m.clip_session(frames, flow_frames)
    for i, (te, se, noise) in enumerate(qs):
        ref = m.generate(frames, flow_frames, nframe, te, se, noise=noise, **kw)
        assert_same(sess.generate(nframe, te, se, noise=noise, **kw), ref, f"full-size question {i}")
    del m, lm, sess
    torch.cuda.empty_cache()


def test_session_is_stale_after_weight_or_dtype_changes(dev, tiny_sd):
    m, cfg, sd = build("instructblip", tiny_sd, dev, "f32")
    T, nframe = 12, 4
    frames, flow_frames = clip(cfg, dev, T)
    (te, se, noise), = questions("instructblip", cfg, dev, [(5, 5, 5)], T)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=3)
    sess = m.clip_session(frames, flow_frames)
    sess.generate(nframe, te, se, noise=noise, **kw)
    m.load_state_dict(sd, strict=False)
    with pytest.raises(RuntimeError, match="stale"):
        sess.generate(nframe, te, se, noise=noise, **kw)
    sess = m.clip_session(frames, flow_frames)
    sess.generate(nframe, te, se, noise=noise, **kw)
    m.set_compute_dtype("bf16")
    with pytest.raises(RuntimeError, match="stale"):
        sess.generate(nframe, te, se, noise=noise, **kw)
    sess = m.clip_session(frames, flow_frames)
    with torch.no_grad():
        m.temporal_encoder.mrc_head.bias.add_(0.0)                  # an optimizer step's in-place update
    with pytest.raises(RuntimeError, match="stale"):
        sess.generate(nframe, te, se, noise=noise, **kw)


def test_session_host_validation(dev, tiny_sd):
    m, cfg, _ = build("instructblip", tiny_sd, dev, "f32")
    T, N = 12, 8
    frames, flow_frames = clip(cfg, dev, T, N)
    with pytest.raises(ValueError):
        m.clip_session(torch.cat([frames, frames]).view(2, N, 3, 56, 56), flow_frames)
    with pytest.raises(ValueError):
        m.clip_session(frames, torch.cat([flow_frames, flow_frames]))
    sess = m.clip_session(frames, flow_frames)
    (te, se, noise), (te2, se2, _) = questions("instructblip", cfg, dev, [(5, 5, 5), (5, 5, 5)], T)
    both = BE({k: torch.cat([se[k], se2[k]]) for k in se})
    with pytest.raises(ValueError):
        sess.generate(4, te, both, max_new_tokens=2)
    with pytest.raises(ValueError):
        sess.generate(N + 1, te, se, noise=noise, max_new_tokens=2)
