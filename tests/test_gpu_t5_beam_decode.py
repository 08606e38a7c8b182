"""-m gpu: beam search on the T5 graph decoder (opt-in: beam_search="graph+t5") on the device -- the captured step over
vtgb_llm_attention_rows_beam (self-attention through the ancestry table), vtgb_llm_attention_rows{,_masked} with rows_per_batch = K (the
encoder's K | V once per batch item) and vtgb_llm_beam_candidates.  fp32 ids against HF ``generate`` (transformers' ``_beam_search`` over an
encoder-decoder) on the device, token for token, for the main cases of tests/test_t5_beam_decode.py at d_kv 16 and 64; at bf16 the decoder
against itself (replay = eager steps, a batch = its rows alone, two runs); and the BLIP-2 LightningModule twin with the shipped
``generate_configs``, with "graph+t5", with "graph" and without the option.  The language model is the tiny T5 of tests/test_decode.py with
lm_head x 4: the beams' log-probabilities spread and beams really re-order."""
import functools
import warnings

import pytest
import torch
from torch.profiler import ProfilerActivity, profile

from conftest import full_state_dict, load_golden, write_hf_config

pytestmark = pytest.mark.gpu

N_NEW, P, D = 20, 7, 64
SHIPPED_SF = dict(length_penalty=1, repetition_penalty=1.5, num_beams=5, min_length=1, max_length=250)      # LSTP_SF_blip2.yaml / LSTP_TG_blip2.yaml
ATTN_KERNEL, CAND_KERNEL = "llm_attn_rows_beam_kernel", "beam_row_kernel"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


@functools.lru_cache(maxsize=None)
def _lm(dev, dtype, dk):
    from transformers import T5Config, T5ForConditionalGeneration
    torch.manual_seed(0)
    cfg = T5Config(vocab_size=200, d_model=D, d_kv=dk, d_ff=96, num_layers=3, num_decoder_layers=3, num_heads=4, feed_forward_proj="gated-gelu",
                   tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    lm = T5ForConditionalGeneration(cfg).eval()
    for p in lm.parameters():
        p.data.normal_(0, 0.3 if dk == 16 else 0.15)      # (scores grow with d_kv: T5 does not scale them)
    with torch.no_grad():
        lm.lm_head.weight.mul_(4.0)
    return lm.to(device=dev, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _decoder(dev, dtype, dk):
    from videotgb_amd.decode import T5GreedyDecoder
    return T5GreedyDecoder(_lm(dev, dtype, dk))


@functools.lru_cache(maxsize=None)
def _inputs(dev, dtype, B):
    g = torch.Generator().manual_seed(5 + B)
    x = (torch.randn(B, P, D, generator=g) * 0.5).to(dev, dtype)
    m = torch.ones(B, P, dtype=torch.long)
    if B > 1:
        m[1, -2:] = 0      # a padded encoder row
    return x, m.to(dev)


def _hf(lm, x, m, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return lm.generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, **kw)


@functools.lru_cache(maxsize=None)
def _eos_ids(dev, dk, B, K):
    """eos ids chosen from what the model emits (the first distinct tokens of the unconstrained search's output)."""
    x, m = _inputs(dev, torch.float32, B)
    free = _hf(_lm(dev, torch.float32, dk), x, m, num_beams=K, repetition_penalty=1.5, max_new_tokens=N_NEW, eos_token_id=None)
    seen = []
    for t in free[:, 1:].flatten().tolist():
        if t not in seen and t != 0:
            seen.append(t)
    return tuple(seen[:3])


def _beam_state(dec):
    st = next(reversed(dec.graphs.values()))
    assert st["attn"] == "beam" and st["beam"]["kernel"] and st["hip"]
    return st


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dk", [16, 64])
def test_fp32_ids_equal_hf_generate(dev, dk, B, K):
    lm, dec = _lm(dev, torch.float32, dk), _decoder(dev, torch.float32, dk)
    x, m = _inputs(dev, torch.float32, B)
    ended = full = False
    for eos in (None,) + _eos_ids(dev, dk, B, K):
        kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=eos)
        ref = _hf(lm, x, m, max_new_tokens=N_NEW, **kw)
        out = dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw)
        st = _beam_state(dec)
        assert st["graph"] is not None                                    # the captured step, replayed
        assert st["ckv"][0].shape[0] == B and st["kc"][0].shape[0] == B * K      # the encoder's K | V once per item, the caches per beam row
        assert out.tolist() == ref.tolist(), (dk, B, K, eos)
        if eos is not None:
            has = (ref[:, 1:] == eos).any(-1)
            ended |= bool(has.any())
            full |= bool((~has).any())
        else:
            full |= ref.shape[1] == 1 + N_NEW
    assert ended and full, "over these requests at least one row ends early and at least one runs to the end"
    if K == 5 and B == 3:      # the winning beams were re-ordered: the ancestry table is not the identity
        bi = st["beam_bi"][:, 0]
        assert ((bi % K)[:, 1:] != 0).any()


@pytest.mark.parametrize("length_penalty", [0.0, 2.0])
def test_fp32_length_penalty_min_new_tokens_and_the_shipped_dict(dev, length_penalty):
    from videotgb_amd import decode
    dk, B, K = 64, 3, 3
    lm, dec = _lm(dev, torch.float32, dk), _decoder(dev, torch.float32, dk)
    x, m = _inputs(dev, torch.float32, B)
    eos = _eos_ids(dev, dk, B, K)[0]
    kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=length_penalty, eos_token_id=eos)
    assert dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw).tolist() == _hf(lm, x, m, max_new_tokens=N_NEW, **kw).tolist()
    kw = dict(kw, min_new_tokens=10, repetition_penalty=1.0)
    ref = _hf(lm, x, m, max_new_tokens=N_NEW, **kw)
    assert dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw).tolist() == ref.tolist() and not (ref[:, 1:11] == eos).any()
    if length_penalty == 0.0:      # the shipped dictionary through graph_generate, with max_length / min_length
        cfgs = dict(SHIPPED_SF, max_length=1 + N_NEW, min_length=4)
        owner = type("Owner", (), dict(beam_search="graph+t5"))()
        out = decode.graph_generate(owner, lm, x, m, cfgs)
        assert out is not None and out.tolist() == _hf(lm, x, m, **cfgs).tolist()
        _beam_state(owner._decoder)
        assert decode.graph_generate(type("Owner", (), dict(beam_search="graph"))(), lm, x, m, cfgs) is None


def test_bf16_replay_eager_batch_and_repeat(dev):
    dec = _decoder(dev, torch.bfloat16, 64)
    kw = dict(num_beams=5, repetition_penalty=1.5, eos_token_id=1, pad_token_id=0)
    x, m = _inputs(dev, torch.bfloat16, 3)
    x2 = x[:2].contiguous()
    out = dec.generate(x2, N_NEW, **kw)
    st = _beam_state(dec)
    assert st["graph"] is not None and st["tok"].shape[0] == 10           # B * K = 10 rows: the skinny weight stream (d_model 64 takes it)
    assert torch.equal(dec.generate(x2, N_NEW, **kw), out)                # two runs
    assert torch.equal(dec.generate(x2, N_NEW, use_graph=False, **kw), out)      # eager stepping
    rows = [dec.generate(x2[b: b + 1].contiguous(), N_NEW, **kw) for b in range(2)]
    for b in range(2):                                                    # (a row alone is cropped to its own length: the batch pads it with the fill value)
        r = rows[b][0]
        assert torch.equal(out[b, : r.numel()], r) and (out[b, r.numel():] == 1).all() and r.numel() <= out.shape[1]
    outp = dec.generate(x, N_NEW, attention_mask=m, **kw)                 # a padded batch: replay = eager steps
    assert torch.equal(dec.generate(x, N_NEW, attention_mask=m, use_graph=False, **kw), outp)


def test_what_the_device_path_refuses(dev):
    from videotgb_amd import ops
    dec = _decoder(dev, torch.bfloat16, 64)
    x, _ = _inputs(dev, torch.bfloat16, 1)
    with pytest.raises(NotImplementedError, match="new tokens"):
        dec.generate(x, ops.ATTENTION_ROWS_BEAM_MAX_KEYS + 1, num_beams=2)


# ------------------------------------------------------------------------------------------------------------------- a module twin
class BE(dict):
    __getattr__ = dict.get


def _kernel_names(fn):
    """(result, names of the kernels launched); device activity only: recording every host-side op of HF's 249 eager steps takes 16 s"""
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, {e.key for e in prof.key_averages()}


def _sf_blip2_module(dev, tmp_path, **kw):
    from videotgb_amd import models, modules
    from videotgb_amd.synth import tiny_cfg
    cfg = tiny_cfg("blip2")
    base = write_hf_config(str(tmp_path / "blip2-tiny"), "blip2", cfg, "t5")
    sd = full_state_dict(cfg, models.build_language_model(models.load_hf_config(base, "blip2")))
    raft_pth = str(tmp_path / "raft-things.pth")
    torch.save({"module." + k[len("of_extractor."):]: v for k, v in sd.items() if k.startswith("of_extractor.")}, raft_pth)
    proc = BE(tokenizer=BE(pad_token_id=0), batch_decode=lambda ids, skip_special_tokens=True: [" ".join(map(str, r)) for r in ids.tolist()])
    m = modules.LSTPSFBlip2Module(model_name_or_path=base, sampler_name_or_path=str(tmp_path / "no-bert-weights"), of_extractor_name_or_path=raft_pth,
                                  temperature=1.0, generate_configs=dict(SHIPPED_SF), compute_dtype="f32", processor=proc, tgb_cfg=cfg.tgb, **kw)
    m.load_state_dict(sd, strict=True)
    m.to(dev)
    with torch.no_grad():
        m.model.language_model.lm_head.weight.mul_(4.0)
    g = load_golden("tiny_modules")
    up4 = lambda q: q.float().repeat_interleave(4, -2).repeat_interleave(4, -1)      # noqa: E731
    B = 2
    batch = dict(frames=(up4(g["frames_q8"]) / 48).to(dev), nframe=int(g["nframe"]), of_lengths=g["of_lengths"].tolist(),
                 answer=torch.zeros(B, 1, dtype=torch.long, device=dev), text_answer=[""] * B,
                 sampler_question=g["sfb2_sampler_ids"].to(dev), sampler_question_attention_mask=g["sfb2_sampler_mask"].to(dev),
                 qformer_text=g["sfb2_qformer_ids"].to(dev), qformer_text_attention_mask=g["sfb2_qformer_mask"].to(dev),
                 question=g["sfb2_question"].to(dev), question_attention_mask=g["sfb2_question_mask"].to(dev),
                 of=(up4(g["of_q8"]) / 127).to(dev), of_mask=g["of_mask"].to(dev))
    return m, batch, (g["sfb2_noise"].to(dev) if "sfb2_noise" in g else None)


def test_sf_blip2_module_eval_forward_with_the_shipped_generate_configs(dev, tmp_path):
    """Without the option and with "graph": HF generate (no decoder is built; under "graph" neither beam kernel is launched).
    beam_search="graph+t5": the same ids at fp32, on the new attention kernel and the candidates kernel, without a BLAS kernel."""
    m, batch, noise = _sf_blip2_module(dev, tmp_path)
    assert m.beam_search == "hf"
    ref = m.eval_forward(batch, noise=noise)                                     # the default: HF generate
    assert getattr(m, "_decoder", None) is None and ref.shape[1] > 1 and (ref[:, 0] == 0).all()
    m.beam_search = "graph"                                                      # the Llama opt-in leaves a T5's beams on HF
    ids, names = _kernel_names(lambda: m.eval_forward(batch, noise=noise))
    assert getattr(m, "_decoder", None) is None and ids.tolist() == ref.tolist()
    assert any("Cijk_" in n for n in names), sorted(names)[:60]                  # (the profile does see HF's kernels)
    assert not any(ATTN_KERNEL in n or CAND_KERNEL in n or "beam_merge_kernel" in n for n in names)
    m.beam_search = "graph+t5"
    ids, names = _kernel_names(lambda: m.eval_forward(batch, noise=noise))
    assert getattr(m, "_decoder", None) is not None and _beam_state(m._decoder)["beam"]["K"] == 5
    assert ids.tolist() == ref.tolist()
    assert any(ATTN_KERNEL in n for n in names) and any(CAND_KERNEL in n for n in names), sorted(names)[:60]
    blas = sorted(n for n in names if "Cijk_" in n)
    assert not blas, blas
