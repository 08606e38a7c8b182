"""Greedy decode for the LLM at the end of the path, replayed from a hipGraph.

The LLM is third-party on both sides: the reference calls HF
``language_model.generate(inputs_embeds=...)`` one eager forward per token, which on MI355X is
launch-bound (~500 small launches per token).  This module runs the SAME arithmetic (the HF
Llama weights, RMSNorm / rotary / SwiGLU definitions of transformers' modeling_llama) as plain
PyTorch-ROCm ops over a static KV cache and captures ONE decode step -- embedding lookup, all
layers, lm_head, argmax, token/position feedback -- into a hipGraph (torch.cuda.CUDAGraph),
so the N-token loop is N graph replays with no host round trip.  At the batch sizes of the
throughput harness the step is then HBM-bound (13.5 GB of bf16 weights per token for Vicuna-7B).

Scope: Llama-architecture models, padded or unpadded prompts (``attention_mask``: HF's per-row position ids and key masks); greedy, or -- round 6, the reference's own eval call
(eval/inference.py:98-109: ``do_sample=True, temperature=0.2, stopping_criteria=[KeywordsStoppingCriteria(['</s>'])]``) -- temperature / top-k /
top-p SAMPLING by inverse CDF over the warped distribution with one uniform number per (step, row) (drawn on the device, or injected:
``sample_noise``), and keyword STOPPING: the token-suffix half of KeywordsStoppingCriteria (eval/utils/builder_utils.py:333-340) runs inside the
captured step, its text half on the host once per 16 tokens.  Anything else goes through HF generate (models.LSTP.generate).
EOS handling is HF's (GenerationMixin._sample with EosTokenCriteria): a per-sequence finished flag
lives on the device inside the captured step; a finished row emits ``pad_token_id`` from then on, and
the returned ids end at the step where the last row finished.  ``min_new_tokens`` masks the EOS logit
for the first steps like MinNewTokensLengthLogitsProcessor.  ``eos_token_id=None`` = fixed-length
decode (the bench's "no EOS stopping, fixed work per clip" mode).
Greedy ids are checked token-for-token against HF generate at fp32 (tests/test_decode.py, test_gpu_e2e.py).
Opt-in, by six string attributes of a decoder's owner (``MODES`` lists them, their values and what each means; ``DecodeModes`` is their parsed
form): fp8 / MXFP4 weight streams and an fp8 K/V cache on the Llama decoder, HF's deterministic beam search on either decoder (over the fp8 cache
as well), eos-id sets, the twins' sampled ``generate_configs``, a repetition penalty on one beam.  By default every such request goes to HF
generate as before and the decoders are built as before (tests/test_decode_modes.py holds all 240 combinations to that).

Structure: ``_GraphDecoder`` owns everything that is not the model -- the state cache (LRU, MAX_STATES), the emission state (token / position
feedback, finished flags, lengths, sampling and stopping data), token selection, capture, the replay loop and the truncation of the returned ids;
``GreedyDecoder`` (Llama) and ``T5GreedyDecoder`` add weights, prefill / encoder, one decode step and their buffers.  ``plan_decode`` is the one
place that decides "graph decoder or HF generate" (each caller's envelope is an ``Envelope`` value), ``decoder_for`` the one place a decoder is
cached on its owner, ``modes_of`` the one place an owner's mode attributes are read.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _lib as L, ops
from .ops import _ptr, _stream, dtype_code

Tensor = torch.Tensor


def _rms(x: Tensor, w: Tensor, eps: float) -> Tensor:
    # LlamaRMSNorm.forward: fp32 variance, weight * x.to(input_dtype); one fused kernel on the device
    if x.is_cuda:
        return F.rms_norm(x, (x.shape[-1],), w, eps)
    dt = x.dtype
    xf = x.float()
    xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return w * xf.to(dt)


def _rot_half(x: Tensor) -> Tensor:
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


# An owner's opt-in switches (attributes of a models.LSTP, a LightningModule twin or any object handed to ``decoder_for`` / ``envelope_for``),
# each with the values it accepts, the default first.  ``modes_of`` reads and parses them; nothing else does.
#   decode_weights  the weights the Llama decoder streams: "bf16" (the model's own), "fp8" (per-row e4m3 codes) or "mxfp4" (e2m1 codes under an
#                   E8M0 scale per 32 weights)
#   kv_cache        the Llama decoder's K/V cache: "bf16" (the model's own K/V) or "fp8" (per-row e4m3 codes)
#   beam_search     who runs a beam-search request: "hf" (HF generate), "graph" (the Llama graph decoder; a T5's beam requests stay on HF),
#                   "graph+t5" (that, and the T5 graph decoder) or either with "+kv8" (that, and the beams of a ``kv_cache="fp8"`` Llama run over
#                   the fp8 cache -- ``GreedyDecoder(fp8_beams=True)`` -- instead of being refused)
#   eos_sets        who runs a request with several distinct eos ids: "hf" or "graph" (the graph decoders, up to ``ops.EOS_MAX`` ids --
#                   ``GreedyDecoder(eos_sets=True)`` / ``T5GreedyDecoder(eos_sets=True)``)
#   sampled_decode  who runs a LightningModule twin's sampled ``generate_configs``: "hf" or "graph" (the module envelope serves ``do_sample`` with
#                   temperature / top_p and takes the length as HF's ``max_length`` / ``min_length`` -- the literal dictionaries of the reference's
#                   LSTP_blip2.yaml / LSTP_instructblip.yaml family -- so that on a Llama they stay on the graph decoder's sampling path; a T5's
#                   sampled requests stay on HF generate)
#   penalty_decode  who runs a ONE-beam request with ``repetition_penalty != 1``: "hf" or "graph" (the graph decoders -- ``GreedyDecoder(penalty=
#                   True)`` / ``T5GreedyDecoder(penalty=True)`` -- apply HF's RepetitionPenaltyLogitsProcessor inside the captured step: greedy on
#                   both, sampling on a Llama).  Beams keep their own penalty (``beam_search``)
MODES = {"decode_weights": ("bf16", "fp8", "mxfp4"),
         "kv_cache": ("bf16", "fp8"),
         "beam_search": ("hf", "graph", "graph+t5", "graph+kv8", "graph+t5+kv8"),
         "eos_sets": ("hf", "graph"),
         "sampled_decode": ("hf", "graph"),
         "penalty_decode": ("hf", "graph")}


def check_mode(name: str, value) -> str:
    """``value`` when it is one of ``MODES[name]``; ValueError otherwise (anything that is no string included)."""
    if value not in MODES[name]:
        raise ValueError(f"{name} must be one of {MODES[name]}, got {value!r}")
    return value


class DecodeModes(NamedTuple):
    """An owner's six ``MODES`` strings, parsed.  The first five fields are ``GreedyDecoder``'s constructor keywords (``DECODER_MODES``;
    ``T5GreedyDecoder`` takes all but ``fp8_beams``), the last three with ``eos_sets`` and ``penalty`` shape the owner's ``Envelope``."""
    weights: str = "bf16"        # decode_weights
    kv_cache: str = "bf16"
    fp8_beams: bool = False      # beam_search has "+kv8"
    eos_sets: bool = False       # eos_sets is "graph"
    penalty: bool = False        # penalty_decode is "graph"
    beams: bool = False          # beam_search starts with "graph"
    t5_beams: bool = False       # beam_search has "+t5"
    sampled: bool = False        # sampled_decode is "graph"


DECODER_MODES = DecodeModes._fields[:5]


def modes_of(owner) -> DecodeModes:
    """The modes of ``owner``, read from its attributes on every call (callers reassign them between calls); an attribute it lacks takes the
    default, any other value than ``MODES`` lists is a ValueError."""
    weights, kv_cache, beam_search, eos_sets, sampled, penalty = (check_mode(name, getattr(owner, name, values[0])) for name, values in MODES.items())
    beam = beam_search.split("+")      # "graph+t5+kv8" -> who runs beams, on a T5 as well, over the fp8 cache as well
    return DecodeModes(weights, kv_cache, "kv8" in beam, eos_sets == "graph", penalty == "graph", beam[0] == "graph", "t5" in beam, sampled == "graph")


def _first_eos(eos):
    """The id HF's defaults take from a request's eos: the id itself, or the first of a set."""
    return eos[0] if isinstance(eos, tuple) else eos


def weights_key(lm):
    """(in-place version, storage address) of every parameter: the decoders hold re-packed COPIES of the language model's weights
    (concatenated q|k|v, tiled decode weights, captured graphs), so an optimizer step, a load_state_dict or a `.data` swap on
    the model must retire the decoder (round-3 ADVICE) -- ``decoder_for`` compares this key before every use."""
    return tuple((p._version, p.data_ptr()) for p in lm.parameters())


_LORA_PROJECTIONS = ("q_proj", "k_proj", "v_proj")
_T5_LORA_PROJECTIONS = ("q", "k", "v")


def _t5_attentions(lm):
    """The attention modules of a T5 whose q / k / v the T5 graph decoder applies adapters on: every encoder block's SelfAttention, every
    decoder block's SelfAttention and EncDecAttention."""
    out = []
    for stack, idx in ((getattr(lm, "encoder", None), (0,)), (getattr(lm, "decoder", None), (0, 1))):
        for blk in getattr(stack, "block", None) or ():
            for i in idx:
                att = blk.layer[i]
                out.append(getattr(att, "SelfAttention", None) or getattr(att, "EncDecAttention", None))
    return [a for a in out if a is not None]


def _lora_modules(lm):
    """(name, module) of every module that carries adapters (``lora_A`` / ``lora_B`` children, peft's layout; an object that is no
    nn.Module has no modules)."""
    if not isinstance(lm, torch.nn.Module):
        return []
    return [(n, m) for n, m in lm.named_modules() if hasattr(m, "lora_A") or hasattr(m, "lora_B")]


def lora_state(lm) -> Optional[str]:
    """None: ``lm`` has no LoRA adapters; "ok": the graph decoders serve its adapters (train.LoraLinear on q_proj / k_proj / v_proj of a
    Llama's attention layers, or on q / k / v of a T5's ``_t5_attentions``: fp32 "default" adapters, no bias, no active dropout), unmerged, as
    LoraLinear.forward computes them; any other string: why they do not (on a T5 it names the T5) -- the decoders raise NotImplementedError
    with it and ``plan_decode`` hands the request to HF generate, which runs the modules' own forward.  Never "decoded as the base model"."""
    mods = _lora_modules(lm)
    if not mods:
        return None
    if getattr(lm.config, "model_type", "") == "t5":
        served = {id(getattr(att, p, None)) for att in _t5_attentions(lm) for p in _T5_LORA_PROJECTIONS}
        why = _lora_refusal(lm, mods, served, "adapters outside q / k / v of the encoder's and the decoder's SelfAttention and the decoder's EncDecAttention")
        return "ok" if why is None else f"LoRA adapters on a T5 language model -- {why}"
    layers = getattr(getattr(lm, "model", None), "layers", None) or ()
    served = {id(getattr(l.self_attn, p, None)) for l in layers if hasattr(l, "self_attn") for p in _LORA_PROJECTIONS}
    return _lora_refusal(lm, mods, served, "adapters outside q_proj / k_proj / v_proj of the attention layers") or "ok"


def _lora_refusal(lm, mods, served, outside: str) -> Optional[str]:
    """Why the adapter-carrying modules ``mods`` are not all servable LoraLinears among ``served`` (ids), or None."""
    from .train import LoraLinear
    for name, m in mods:
        if not isinstance(m, LoraLinear):
            return f"{name}: adapters on a {type(m).__name__}, not a videotgb_amd.train.LoraLinear"
        if id(m) not in served:
            return f"{name}: {outside}"
        if "default" not in m.lora_A or "default" not in m.lora_B:
            return f"{name}: no \"default\" adapter"
        A, B = m.lora_A["default"].weight, m.lora_B["default"].weight
        if A.dtype != torch.float32 or B.dtype != torch.float32:
            return f"{name}: adapters are {A.dtype} / {B.dtype}, not fp32"
        if m.bias is not None or m.lora_A["default"].bias is not None or m.lora_B["default"].bias is not None:
            return f"{name}: a LoraLinear with a bias"
        p = float(getattr(m.lora_dropout["default"], "p", 0.0)) if "default" in m.lora_dropout else 0.0
        if (lm.training or m.training) and p > 0.0:
            return f"{name}: training mode with lora_dropout={p} (HF generate applies the dropout; call .eval())"
        if not 1 <= A.shape[0] <= L.LORA_MAX_RANK:
            return f"{name}: rank {A.shape[0]} outside 1..{L.LORA_MAX_RANK}"
    return None


def _lora_servable(lm) -> bool:
    """NotImplementedError(reason) for adapters the decoders do not serve; whether there are adapters to apply."""
    state = lora_state(lm)
    if state not in (None, "ok"):
        raise NotImplementedError(f"LoRA adapters outside the graph decoder's envelope -- {state}")
    return state == "ok"


ROPE_TYPES = ("default", "linear", "llama3", "yarn")      # rotary tables that depend on the position alone


def _rope_type(lm) -> str:
    """The rope type of a Llama: the rotary module's own, else the configuration's (``rope_parameters``; ``rope_scaling`` with its older
    ``type`` key), else "default"."""
    cfg = getattr(lm, "config", None)
    rot = getattr(getattr(lm, "model", None), "rotary_emb", None)
    rp = getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None) or {}
    t = getattr(rot, "rope_type", None) or (rp.get("rope_type") or rp.get("type") if isinstance(rp, dict) else None)
    return str(t or "default")


def llama_state(lm) -> Optional[str]:
    """None: ``GreedyDecoder`` states this Llama -- plain or position-only scaled rotary embedding (``ROPE_TYPES``, tables built from the model's own
    ``rotary_emb.inv_freq`` and ``attention_scaling``), with or without projection biases (``attention_bias`` / ``mlp_bias``).  Any string: what
    the layer statement does not compute -- the decoder raises NotImplementedError with it and ``plan_decode`` hands the request to HF generate.
    An attribute a stand-in object lacks counts as a default Llama's.  Never "decoded as a plain Llama"."""
    cfg = getattr(lm, "config", None)
    mt = getattr(cfg, "model_type", "")
    if mt != "llama":
        return f"model_type {mt!r}: the layer statement is LlamaForCausalLM's"
    rt = _rope_type(lm)
    if rt not in ROPE_TYPES:
        return f"rope_type {rt!r}: rotary tables that depend on the running sequence length, or unknown ones, are not built (served: {ROPE_TYPES})"
    rot = getattr(getattr(lm, "model", None), "rotary_emb", None)
    if rt != "default":
        inv = getattr(rot, "inv_freq", None)
        if not isinstance(inv, Tensor):
            return f"rope_type {rt!r} on a model without rotary_emb.inv_freq to build the tables from"
        nh = getattr(cfg, "num_attention_heads", None)
        hd = getattr(cfg, "head_dim", None) or (cfg.hidden_size // nh if nh else None)
        if hd is not None and inv.numel() * 2 != hd:
            return f"rotary_emb.inv_freq of {inv.numel()} frequencies for head_dim {hd} (partial rotary embedding)"
    act = getattr(cfg, "hidden_act", "silu")
    if act not in ("silu", "swish"):
        return f"hidden_act {act!r}: the MLP statement is SwiGLU"
    if getattr(getattr(lm, "lm_head", None), "bias", None) is not None:
        return "an lm_head with a bias"
    layers = getattr(getattr(lm, "model", None), "layers", None) or ()
    for li, l in enumerate(layers):      # anything but the norm -> attention -> norm -> MLP layer of modeling_llama
        a, m = getattr(l, "self_attn", None), getattr(l, "mlp", None)
        missing = [p for p in ("q_proj", "k_proj", "v_proj", "o_proj") if not hasattr(a, p)] + [p for p in ("gate_proj", "up_proj", "down_proj") if not hasattr(m, p)]
        if missing:
            return f"layer {li} without {missing[0]}"
        for n in ("q_norm", "k_norm"):
            if hasattr(a, n):
                return f"layer {li}: self_attn.{n}"
    return None


def _llama_servable(lm):
    state = llama_state(lm)
    if state is not None:
        raise NotImplementedError(f"a Llama outside the graph decoder's statement -- {state}; use HF generate")


def prefill_chunks(P: int, chunk: int):
    """The chunked prefill's plan: [(q0, n), ...] -- consecutive row ranges [q0, q0 + n) covering 0 .. P-1, every n == chunk but the last."""
    if P <= 0 or chunk <= 0:
        raise ValueError(f"prefill_chunks: P={P} and chunk={chunk} must be positive")
    return [(q0, min(chunk, P - q0)) for q0 in range(0, P, chunk)]


def _padding(attention_mask: Optional[Tensor], B: int, P: int) -> Optional[Tensor]:
    """The decoders' view of a prompt mask: None when there is none or it is all ones (the unpadded path, unchanged), else the mask.
    Rejects what HF would not decode the same way here: a shape other than [B, P], values other than 0 / 1, a row without a token."""
    if attention_mask is None:
        return None
    if tuple(attention_mask.shape) != (B, P):
        raise ValueError(f"attention_mask of shape {tuple(attention_mask.shape)} for inputs_embeds of {B} x {P} positions")
    padded, host = prompt_padding(attention_mask)
    if padded is None:
        raise ValueError("attention_mask: 0 / 1 values and at least one token per row")
    return host if padded else None


class _GraphDecoder:
    """The model-independent half of both decoders.  A subclass supplies ``_state`` (its key and buffers, through ``_cached_state``),
    ``_decode_step(st)`` (one token for every row, ending in ``_emit``) and ``generate``: prefill, ``_reset``, then ``_replay``."""
    MAX_STATES = 4
    FEEDBACK = ("tok", "pos", "step", "out", "fin", "len")      # what one step writes besides the model's caches

    # a one-beam repetition penalty on the fused device path: True = ops.repetition_penalty (vtgb_llm_repetition_penalty) into the state's fp32
    # buffer; False = the torch statement of ``_penalise`` (what every other path runs) -- the switch of the A/B (tools/penalty_decode_bench.py)
    PENALTY_KERNEL = True

    def __init__(self, lm, fused: bool, weights: str = "bf16", kv_cache: str = "bf16", eos_sets: bool = False, penalty: bool = False):
        self.lm, self.cfg, self.fused, self.weights = lm, lm.config, fused, check_mode("decode_weights", weights)
        self.kv_cache = check_mode("kv_cache", kv_cache)
        self.eos_sets = bool(eos_sets)      # opt-in (eos_sets="graph"): requests with 2 .. ops.EOS_MAX distinct eos ids instead of a refusal
        self.penalty = bool(penalty)        # opt-in (penalty_decode="graph"): one beam with repetition_penalty != 1 instead of a refusal
        self.key = weights_key(lm)
        self.graphs: Dict[tuple, dict] = {}

    def _special(self, eos_token_id, pad_token_id, min_new_tokens):
        """(eos, pad, min_new) as the state holds them: a one-element eos list unwrapped, HF's pad default (the eos id), ints.  A decoder built
        with ``eos_sets``: a list of 2 .. ops.EOS_MAX distinct ids in [0, V) stays a tuple in the caller's order, duplicates dropped (HF's pad
        default is then its first id); a list that collapses to one id is that id."""
        if isinstance(eos_token_id, (list, tuple)):
            ids = tuple(dict.fromkeys(int(v) for v in eos_token_id)) if self.eos_sets and len(eos_token_id) > 0 else tuple(eos_token_id)
            if len(ids) != 1:
                V = self.lm.lm_head.weight.shape[0]
                if not self.eos_sets or not 2 <= len(ids) <= ops.EOS_MAX or any(not 0 <= v < V for v in ids):
                    raise NotImplementedError(f"{type(self).__name__}: one eos_token_id" + (
                        f", or (eos_sets) 2 .. {ops.EOS_MAX} distinct ids in [0, {V})" if self.eos_sets else ""))
                return ids, int(pad_token_id if pad_token_id is not None else ids[0]), int(min_new_tokens or 0)
            eos_token_id = ids[0]
        return eos_token_id, int(pad_token_id if pad_token_id is not None else (eos_token_id or 0)), int(min_new_tokens or 0)

    def _one_beam_penalty(self, repetition_penalty) -> float:
        """The penalty a one-beam state holds: 1.0 (none), or -- a decoder built with ``penalty`` -- the request's; today's refusal otherwise."""
        p = float(repetition_penalty)
        if p != 1.0 and not self.penalty:
            raise NotImplementedError("repetition_penalty with one beam: use HF generate")
        return p

    def _cached_state(self, key: tuple, B: int, N: int, n_ar: int, device, eos, pad: int, min_new: int, sample, stop, buffers: Callable[[], dict],
                      penalty: float = 1.0) -> dict:
        """The state under ``key``, most recently used last; a new one takes the least recently used state's place once MAX_STATES are kept
        (its graph and buffers are freed first) and is the emission state below plus the model's ``buffers()``.  ``penalty`` != 1 (one beam):
        the key gets it -- the captured step bakes the scalar in -- and the state its operands (``_penalise``)."""
        if penalty != 1.0:
            key = key + (("penalty", penalty),)
        st = self.graphs.pop(key, None)
        if st is None:
            while len(self.graphs) >= self.MAX_STATES:
                self.graphs.pop(next(iter(self.graphs))).clear()
            st = dict(tok=torch.zeros(B, dtype=torch.long, device=device), pos=torch.zeros(1, dtype=torch.long, device=device),
                      step=torch.zeros(1, dtype=torch.long, device=device), out=torch.zeros(B, N, dtype=torch.long, device=device),
                      fin=torch.zeros(B, dtype=torch.bool, device=device), ar=torch.arange(n_ar, device=device), graph=None,
                      eos=eos, pad=pad, min_new=min_new, sample=sample, stop=stop,
                      stop_t=[torch.tensor(t, dtype=torch.long, device=device) for t in (stop or ())],      # (device copies made outside any capture)
                      # sampling: one uniform number per (step, row); the generated length of every row (N = not finished)
                      u=torch.zeros(N, B, device=device), len=torch.full((B,), N, dtype=torch.long, device=device))
            if isinstance(eos, tuple):      # an eos set: its device list (isin on the torch path, the kernels' operand on the fused one)
                st["eos_t"] = torch.tensor(eos, dtype=torch.int32, device=device)
            if penalty != 1.0:      # the scalar, its fp32 tensor (a tensor divisor is a true division on every backend) and, where the kernel runs, its output
                st.update(pen=penalty, pen_t=torch.tensor([penalty], dtype=torch.float32, device=device))
                if self.fused and torch.device(device).type == "cuda":
                    st["pen_out"] = torch.zeros(B, self.lm.lm_head.weight.shape[0], dtype=torch.float32, device=device)
            st.update(buffers())
        self.graphs[key] = st
        return st

    def _pick(self, st, logits: Tensor, step) -> Tensor:
        """Next token of every row with HF's EOS semantics (device-side, capturable): EOS masked while step < min_new_tokens, finished rows emit
        pad, a row finishes when it emits EOS.  Greedy: argmax.  Sampling (``st["sample"] = (temperature, top_k, top_p)``): HF's warpers
        (TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper; GenerationMixin._sample) then the inverse CDF of the warped distribution at
        this step's uniform number -- the distribution of torch.multinomial(softmax(.)), a different random stream (HF's is not reproducible
        across torch versions either); temperature -> 0 degenerates to the greedy token."""
        eos = st["eos"]
        if eos is not None and st["min_new"] > 0:
            blocked = (step < st["min_new"]) if isinstance(step, Tensor) else torch.tensor([step < st["min_new"]], device=logits.device)
            logits = logits.clone()
            for e in (eos if isinstance(eos, tuple) else (eos,)):      # (an eos set: every id of it)
                logits[:, e] = torch.where(blocked, torch.full_like(logits[:, e], float("-inf")), logits[:, e])
        if st["sample"] is None:
            nxt = logits.argmax(-1)
        else:
            temperature, top_k, top_p = st["sample"]
            k = min(int(top_k), logits.shape[-1]) if top_k else logits.shape[-1]
            vals, idx = (logits.float() / temperature).topk(k, dim=-1)                  # sorted, largest first
            p = torch.softmax(vals, -1)
            if top_p is not None and top_p < 1.0:                                        # nucleus: the smallest prefix whose mass reaches top_p
                keep = (p.cumsum(-1) - p) < top_p
                p = torch.where(keep, p, torch.zeros_like(p))
                p = p / p.sum(-1, keepdim=True)
            u = st["u"][step] if not isinstance(step, Tensor) else st["u"].index_select(0, step)[0]
            j = (p.cumsum(-1) < u[:, None]).sum(-1).clamp_(max=k - 1)
            nxt = idx.gather(-1, j[:, None])[:, 0]
        if eos is not None or st["stop"] is not None:
            nxt = torch.where(st["fin"], torch.full_like(nxt, st["pad"]), nxt)
        if isinstance(eos, tuple):
            st["fin"].logical_or_(torch.isin(nxt, st["eos_t"]))
        elif eos is not None:
            st["fin"].logical_or_(nxt == eos)
        return nxt

    def _after_token(self, st, step):
        """Bookkeeping behind the token written to out[:, step]: the keyword-suffix test of KeywordsStoppingCriteria (builder_utils.py:337-339:
        the last len(k) generated ids equal keyword k's ids) and the finished rows' lengths -- on the device, inside the captured step."""
        stop = st["stop"]
        if stop is not None:
            n = max(len(t) for t in stop)
            ar = st["ar"][:n]
            pos = step - (n - 1) + ar                                                    # the last n positions, right-aligned
            window = st["out"].index_select(1, pos.clamp(min=0))
            hit = torch.zeros_like(st["fin"])
            for t, tail in zip(stop, st["stop_t"]):
                ok = (window[:, n - len(t):] == tail[None]).all(-1) & (pos[n - len(t)] >= 0)
                hit = hit | ok
            st["fin"].logical_or_(hit)
        if st["eos"] is not None or stop is not None:
            N = st["out"].shape[1]
            st["len"].copy_(torch.where(st["fin"] & (st["len"] == N), (step + 1).expand_as(st["len"]), st["len"]))

    def _penalty_start(self) -> Optional[int]:
        """An id HF's processors always see besides the generated ones (T5: the decoder start token); None: none."""
        return None

    def _penalise(self, st, logits: Tensor) -> Tensor:
        """HF's RepetitionPenaltyLogitsProcessor on fp32 scores over the ids a row has generated so far (``out[:, :step]``, + ``_penalty_start``):
        x < 0 ? x * p : x / p at every seen index, once.  On the fused device path ops.repetition_penalty into the state's buffer; elsewhere
        (and under ``PENALTY_KERNEL = False``) the fixed-shape statement: ids behind the step go to a spare column, gather / scatter."""
        start, N, V = self._penalty_start(), st["out"].shape[1], logits.shape[-1]
        if "pen_out" in st and self.PENALTY_KERNEL and logits.is_cuda and logits.dtype in (torch.bfloat16, torch.float32):
            return ops.repetition_penalty(logits, st["out"], st["step"], st["pen"], start, out=st["pen_out"])
        x = logits.float()
        ids = torch.where(st["ar"][None, :N] < st["step"], st["out"], torch.full_like(st["out"], V))
        if start is not None:
            ids = torch.cat((torch.full_like(ids[:, :1], start), ids), dim=1)
        x = torch.cat((x, torch.zeros_like(x[:, :1])), dim=-1)
        g = x.gather(1, ids)
        return x.scatter(1, ids, torch.where(g < 0, g * st["pen_t"], g / st["pen_t"]))[:, :V].contiguous()

    def _emit(self, st, logits: Tensor):
        if "pen" in st:      # (one beam, repetition_penalty != 1) before the eos block of min_new_tokens and the warpers, as in HF
            logits = self._penalise(st, logits)
        if "eos_t" in st and st["sample"] is None and self.fused and logits.is_cuda:
            # an eos set, greedy, on the device: ``_pick`` and the two writes below in one launch (vtgb_llm_pick_greedy)
            ops.pick_greedy(logits, st["step"], st["eos_t"], st["fin"], st["tok"], st["out"], st["min_new"], st["pad"])
        else:
            nxt = self._pick(st, logits, st["step"])
            st["tok"].copy_(nxt)
            st["out"].index_copy_(1, st["step"], nxt[:, None])
        self._after_token(st, st["step"])
        st["pos"].add_(1)
        st["step"].add_(1)

    def _reset(self, st, ending: bool, pos: int):
        """The feedback buffers before a call: nothing finished, step 0 at position ``pos`` (the caller sets ``tok``); ``out`` is pre-filled
        with pad only when rows can end early (otherwise every column is written)."""
        st["fin"].zero_()
        st["len"].fill_(st["out"].shape[1])
        if ending:
            st["out"].fill_(st["pad"])
        st["step"].zero_()
        st["pos"].fill_(pos)

    def _capture(self, st):
        """One decode step into a graph: a warm-up step on a side stream first (handles, workspaces), the feedback buffers put back after both."""
        names = st.get("feedback", self.FEEDBACK)      # (a beam state: its bookkeeping as well)
        keep = [st[k].clone() for k in names]

        def restore():
            for k, v in zip(names, keep):
                st[k].copy_(v)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._decode_step(st)
        torch.cuda.current_stream().wait_stream(s)
        restore()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._decode_step(st)
        st["graph"] = g
        restore()

    def _replay(self, st, first: int, use_graph: bool, ending: bool, text_stop=None) -> Tensor:
        """Steps ``first`` .. N-1 (``first`` tokens were emitted before the loop: Llama's comes from its prefill, T5 starts at 0), one graph replay
        each, with one host read per 16 tokens when rows can end early (never before a step has run); returns ``out`` up to the step where the
        last row finished, as HF does -- ``len.max()``, or the length at which the text test first held."""
        N = st["out"].shape[1]
        use_graph = use_graph and st["tok"].is_cuda
        checked, cut = 0, None        # text test: lengths [1, checked] have been tested; cut = the length at which it first held
        if N > first:
            if use_graph and st["graph"] is None:
                self._capture(st)
            for i in range(N - first):
                if ending and i % 16 == 0 and i + first > 0:
                    if text_stop is not None:
                        cut, checked = self._text_scan(st, text_stop, checked, i + first)
                        if cut is not None:
                            break
                    if bool(st["fin"].all()):
                        break                      # every row has finished
                if use_graph:
                    st["graph"].replay()
                else:
                    self._decode_step(st)
        out = st["out"].clone()
        if text_stop is not None and cut is None:
            cut, checked = self._text_scan(st, text_stop, checked, int(st["step"].item()))
        if ending:
            n = int(st["len"].max().item())
            out = out[:, : n if cut is None else min(n, cut)]
        return out

    # ---- beam search: transformers 5.15.0 GenerationMixin._beam_search and its helpers (_get_top_k_continuations,
    # _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic, _beam_search_has_unfinished_sequences) with
    # fixed shapes and the step as device data, capturable like ``_emit``.  The prompt arrives as embeddings, so HF's ``input_ids`` is empty:
    # cur_len and decoder_prompt_len start at 0, max_length is N, only generated ids feed the repetition penalty.  early_stopping is False.
    # Per-vocabulary work is ops.beam_candidates (vtgb_llm_beam_candidates) on the fused device path and the torch statement elsewhere; the
    # [B, 2K]-sized bookkeeping is torch ops inside the captured step.
    BEAM_BOOK = ("run_seq", "run_scores", "run_bi", "seqs", "beam_scores", "beam_bi", "sent_fin", "unsat", "done")

    def _beam_book(self, B: int, K: int, N: int, device, fill: int) -> dict:
        """The bookkeeping of one beam search over B items, K beams, N new tokens (``_beam_search``, "3. init running tensors")."""
        return dict(run_seq=torch.full((B, K, N), fill, dtype=torch.long, device=device), seqs=torch.full((B, K, N), fill, dtype=torch.long, device=device),
                    run_scores=torch.zeros(B, K, device=device), beam_scores=torch.zeros(B, K, device=device),
                    run_bi=torch.zeros(B, K, N, dtype=torch.int32, device=device), beam_bi=torch.zeros(B, K, N, dtype=torch.int32, device=device),
                    sent_fin=torch.zeros(B, K, dtype=torch.bool, device=device), unsat=torch.ones(B, 1, dtype=torch.bool, device=device),
                    done=torch.zeros(1, dtype=torch.bool, device=device),
                    top_mask=torch.cat((torch.ones(K, dtype=torch.bool), torch.zeros(K, dtype=torch.bool))).to(device),
                    item_off=(torch.arange(B, device=device) * K)[:, None], cand_score=torch.zeros(B, 2 * K, device=device),
                    cand_idx=torch.zeros(B, 2 * K, dtype=torch.int32, device=device))

    def _beam_reset(self, st):
        fill = st["beam"]["fill"]
        st["run_seq"].fill_(fill)
        st["seqs"].fill_(fill)
        st["run_scores"].fill_(-1e9)
        st["run_scores"][:, 0] = 0.0      # only the first beam's tokens count at the first step: the K rows are identical
        st["beam_scores"].fill_(-1e9)
        st["run_bi"].fill_(-1)
        st["beam_bi"].fill_(-1)
        st["sent_fin"].zero_()
        st["unsat"].fill_(True)
        st["done"].zero_()

    def _beam_candidates(self, st, logits: Tensor):
        """(score [B, 2K] fp32, flat index [B, 2K] int64 = k * V + token): log_softmax, the repetition penalty over the ids generated so far,
        the eos block of min_new_tokens, + the running scores, the 2K best per item."""
        bm, step = st["beam"], st["step"]
        B, K, N = st["run_seq"].shape
        V = logits.shape[-1]
        if bm["kernel"] and "eos_t" in st:      # an eos set: the list instantiation of the same kernel
            sc, ix = ops.beam_candidates_eos(logits, st["run_seq"].view(B * K, N), step, st["run_scores"], st["eos_t"], bm["repetition_penalty"],
                                             st["min_new"], out=(st["cand_score"], st["cand_idx"]), workspace=st["cand_ws"])
            return sc, ix.long()
        if bm["kernel"]:
            sc, ix = ops.beam_candidates(logits, st["run_seq"].view(B * K, N), step, st["run_scores"], bm["repetition_penalty"], st["eos"],
                                         st["min_new"], out=(st["cand_score"], st["cand_idx"]), workspace=st["cand_ws"])
            return sc, ix.long()
        lp = F.log_softmax(logits.float(), dim=-1)
        if bm["repetition_penalty"] != 1.0:      # RepetitionPenaltyLogitsProcessor on the log-probabilities; ids behind the step go to a spare column
            ids = torch.where(st["ar"][None, :N] < step, st["run_seq"].view(B * K, N), torch.full_like(st["run_seq"].view(B * K, N), V))
            lp = torch.cat((lp, torch.zeros_like(lp[:, :1])), dim=-1)
            g = lp.gather(1, ids)
            lp = lp.scatter(1, ids, torch.where(g < 0, g * bm["repetition_penalty"], g / bm["repetition_penalty"]))[:, :V]
        if st["eos"] is not None and st["min_new"] > 0:
            lp = lp.clone()
            for e in (st["eos"] if isinstance(st["eos"], tuple) else (st["eos"],)):      # (an eos set: every id of it)
                lp[:, e] = torch.where(step < st["min_new"], torch.full_like(lp[:, e], float("-inf")), lp[:, e])
        acc = (lp.view(B, K, V) + st["run_scores"][:, :, None]).reshape(B, K * V)
        return torch.topk(acc, k=2 * K)

    def _beam_select(self, st, logits: Tensor) -> Tensor:
        """One ``_beam_search`` iteration behind the logits [B*K, V] at cur_len = *step: the bookkeeping is advanced (frozen once ``done``) and
        the next tokens go to ``tok``; returns the rows [B*K] the next beams continue (their parents)."""
        bm, step = st["beam"], st["step"]
        B, K, N = st["run_seq"].shape
        V = logits.shape[-1]
        lpen = bm["length_penalty"]

        def take(t, idx):      # _gather_beams
            while idx.dim() < t.dim():
                idx = idx.unsqueeze(-1)
            return torch.take_along_dim(t, idx, dim=1)

        def over(t, d):        # t / d for a length-penalty denominator: HF divides by a Python scalar (on the device: times its fp32 reciprocal)
            return t * (1.0 / d) if t.is_cuda else t / d
        # c. _get_top_k_continuations
        score, flat = self._beam_candidates(st, logits)
        beam, token = flat // V, flat % V
        at = step.view(1, 1, 1).expand(B, 2 * K, 1)
        top_seq = take(st["run_seq"], beam).scatter(2, at, token[:, :, None])
        top_bi = take(st["run_bi"], beam).scatter(2, at, (beam + st["item_off"]).to(torch.int32)[:, :, None])
        # d. stopping criteria: EosTokenCriteria | MaxLengthCriteria
        hits = (step + 1 >= N).expand(B, 2 * K)
        if "eos_t" in st:
            hits = hits | torch.isin(token, st["eos_t"])
        elif st["eos"] is not None:
            hits = hits | (token == st["eos"])
        # e. _get_running_beams_for_next_iteration
        run_lp = score + hits.to(torch.float32) * -1.0e9
        nxt = torch.topk(run_lp, k=K)[1]
        run_seq, run_scores, run_bi = take(top_seq, nxt), take(run_lp, nxt), take(top_bi, nxt)
        # f. _update_finished_beams (early_stopping False)
        did = hits & st["top_mask"][None, :]
        fin_lp = over(score, torch.pow((step + 1).double(), lpen).float())
        fin_lp = fin_lp + (~st["unsat"]).to(torch.float32) * -1.0e9
        fin_lp = fin_lp + (~did) * -1.0e9
        m_scores = torch.cat((st["beam_scores"], fin_lp), dim=1)
        keep = torch.topk(m_scores, k=K)[1]
        seqs, beam_scores = take(torch.cat((st["seqs"], top_seq), dim=1), keep), take(m_scores, keep)
        beam_bi, sent_fin = take(torch.cat((st["beam_bi"], top_bi), dim=1), keep), take(torch.cat((st["sent_fin"], did), dim=1), keep)
        # g. _check_early_stop_heuristic at cur_len + 1, _beam_search_has_unfinished_sequences
        best = over(run_scores[:, :1], torch.pow((step + 1).double(), lpen).float())
        worst = torch.where(sent_fin, torch.min(beam_scores, dim=1, keepdim=True)[0], torch.full_like(beam_scores, -1.0e9))
        unsat = st["unsat"] & torch.any(best > worst, dim=-1, keepdim=True)
        more = torch.any(unsat) & ~torch.all(hits)
        # HF leaves its loop on the step that finishes: from then on nothing changes
        done = st["done"]
        for name, new in (("run_seq", run_seq), ("run_scores", run_scores), ("run_bi", run_bi), ("seqs", seqs), ("beam_scores", beam_scores),
                          ("beam_bi", beam_bi), ("sent_fin", sent_fin), ("unsat", unsat)):
            st[name].copy_(torch.where(done, st[name], new))
        done.logical_or_(~more)
        st["tok"].copy_(take(token, nxt).reshape(B * K))
        return (take(beam, nxt) + st["item_off"]).reshape(B * K)

    def _beam_result(self, st) -> Tensor:
        """Per batch item the best finished beam, cropped to the longest generated length (counted from ``beam_indices``, as HF does)."""
        n = int(((st["beam_bi"][:, 0] + 1).bool()).sum(dim=1).max().item())
        return st["seqs"][:, 0, :n].clone()

    def _replay_beams(self, st, use_graph: bool) -> Tensor:
        """Steps 1 .. N-1 (the first selection came from the prefill), one graph replay each; ``done`` is read once per 16 steps."""
        N = st["run_seq"].shape[2]
        use_graph = use_graph and st["tok"].is_cuda and st["attn"] in ("beam", "beam_fp8")
        if N > 1:
            if use_graph and st["graph"] is None:
                self._capture(st)
            for i in range(N - 1):
                if i % 16 == 0 and i > 0 and bool(st["done"].item()):
                    break
                if use_graph:
                    st["graph"].replay()
                else:
                    self._decode_step(st)
        return self._beam_result(st)

    @staticmethod
    def _text_scan(st, text_stop, checked: int, upto: int):
        """The criteria's TEXT test for the lengths checked + 1 .. upto (host; the first length at which it holds, or None)."""
        ids = st["out"][:, :upto].cpu()
        for n in range(checked + 1, upto + 1):
            if text_stop(ids[:, :n]):
                return n, n
        return None, upto


class GreedyDecoder(_GraphDecoder):
    """``weights="fp8"`` (opt-in): the seven projections of every layer and lm_head are quantised per output row to e4m3 with a power-of-two scale
    (ops.quantize_fp8_rows) and the decode step streams those codes (ops.SkinnyWeightFp8: half the bytes per token).  ``self.layers`` / ``self.head_w``
    -- what the prefill, batches beyond the skinny kernel and the torch path multiply by -- then hold the DEQUANTISED weights, which are exactly bf16
    numbers, so every path decodes the same model: an ordinary Llama whose projection weights are q * scale.  Embeddings and norms are the
    model's own.  The fused path takes a bf16 model; the torch path (``fused=False``) also an fp32 one, quantised from its bf16 cast.

    ``weights="mxfp4"`` (opt-in): the same arrangement on OCP MXFP4 -- e2m1 codes under one E8M0 scale per 32 weights along K
    (ops.quantize_mxfp4_rows; the decode step streams ops.SkinnyWeightMxfp4, 17 / 64 of the bf16 bytes per token).  code * 2^e is exactly a bf16
    number, so ``self.layers`` / ``self.head_w`` hold the dequantised weights and every path decodes that one model.  Its ids are the quantised
    model's, not the reference's (the format's weight error is 11.5 % rel-RMS on Gaussian rows, fp8's 2.66 %); answer quality on a trained
    checkpoint is not measured by this project.  Same conditions on the model's dtype as fp8.

    ``kv_cache="fp8"`` (opt-in, orthogonal to ``weights``): every K row (after rotary) and every V row -- one token of one K/V head -- is rounded
    once, as it is produced, to e4m3 codes with a power-of-two row scale (ops.quantize_fp8_kv), and the prefill attention, every decode step and
    every fallback attend over the dequantised values, which are exactly bf16 numbers: the mode is an ordinary bf16 Llama whose K/V pass
    through ``ops.fp8_kv_round``.  ``fp8_beams=True`` (opt-in): beam search runs over that cache as well (``_beam_state``) instead of being refused.  On the device, fused, with a cache the split-KV kernel takes (head_dim 64 / 128, up to 16384 slots) the state
    holds the codes and scales (half the bytes: ``st["attn"] == "split_fp8"``, vtgb_llm_rope_cache{,_prefill}_fp8 +
    vtgb_llm_decode_attention_split_fp8); otherwise it keeps bf16 caches of dequantised values and decodes on the torch step (``_layer`` states
    the model; no memory is saved).  The fused path takes a bf16 model; the torch path also an fp32 one.

    Which Llama: ``llama_state`` -- rope types default / linear / llama3 / yarn (scaled types: tables from the model's own rotary module,
    ``_rope``), with or without projection biases (``self.bias``: fp32, never quantised; the decode step adds them in the skinny GEMM's
    epilogue -- ops.gemm_skinny(bias=), vtgb_gemm_skinny_bias --, prefill and large batches through vtgb_gemm's bias, ``_layer`` through
    F.linear).  Anything else raises NotImplementedError with the reason."""

    def __init__(self, lm, fused: bool = True, weights: str = "bf16", kv_cache: str = "bf16", fp8_beams: bool = False, eos_sets: bool = False,
                 penalty: bool = False):
        cfg = lm.config
        if "llama" not in cfg.model_type:
            raise NotImplementedError("GreedyDecoder handles Llama-architecture models; use HF generate otherwise")
        _llama_servable(lm)
        has_lora = _lora_servable(lm)
        super().__init__(lm, fused, weights, kv_cache, eos_sets, penalty)
        self.fp8_beams = bool(fp8_beams)      # opt-in (beam_search="...+kv8"): num_beams > 1 over the fp8 K/V cache; inert with a bf16 cache
        wdt = lm.lm_head.weight.dtype
        if self.kv_cache == "fp8" and wdt != torch.bfloat16 and (fused or wdt != torch.float32):
            raise ValueError(f"kv_cache='fp8' needs a bf16 language model, got {wdt}")
        if self.weights != "bf16" and wdt != torch.bfloat16 and (fused or wdt != torch.float32):
            raise ValueError(f"decode_weights={self.weights!r} needs a bf16 language model, got {wdt}")

        def prep(w):      # the matrix every path multiplies by: the model's own, or (fp8, mxfp4) its dequantised copy
            if self.weights == "bf16":
                return w
            if self.weights == "mxfp4":
                return ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(w.detach().bfloat16()), dtype=w.dtype)
            return ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(w.detach().bfloat16()), dtype=w.dtype)
        self.nh, self.nkv = cfg.num_attention_heads, cfg.num_key_value_heads
        self.hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        self.eps = cfg.rms_norm_eps
        rp = getattr(cfg, "rope_parameters", None) or {}
        self.theta = float(rp.get("rope_theta", getattr(cfg, "rope_theta", 10000.0)))
        # a scaled rotary embedding (linear, llama3, yarn): the model's own frequencies and cos / sin factor, from which ``_rope`` builds the
        # tables as LlamaRotaryEmbedding.forward does; None: the default type, today's formula over ``theta``
        self.rope_scaled = None
        if _rope_type(lm) != "default":
            rot = lm.model.rotary_emb
            self.rope_scaled = (rot.inv_freq.detach().float().clone(), float(getattr(rot, "attention_scaling", 1.0)))
        # fused projection weights (one GEMM for q|k|v, one for gate|up): fewer, larger launches per token
        self.layers = []
        biases = []

        def cat_bias(*mods):      # fp32 [sum of the outputs] (widening is exact; never quantised), or None when none of them has a bias
            bs = [getattr(m, "bias", None) for m in mods]
            if all(b is None for b in bs):
                return None
            return torch.cat([m.weight.new_zeros(m.weight.shape[0], dtype=torch.float32) if b is None else b.detach().float()
                              for m, b in zip(mods, bs)]).contiguous()
        for l in lm.model.layers:
            a, m = l.self_attn, l.mlp
            wqkv = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], dim=0).contiguous()
            wgu = torch.cat([m.gate_proj.weight, m.up_proj.weight], dim=0).contiguous()
            self.layers.append((l.input_layernorm.weight, prep(wqkv), prep(a.o_proj.weight), l.post_attention_layernorm.weight, prep(wgu),
                                prep(m.down_proj.weight)))
            biases.append((cat_bias(a.q_proj, a.k_proj, a.v_proj), cat_bias(a.o_proj), cat_bias(m.gate_proj, m.up_proj), cat_bias(m.down_proj)))
        # per layer the fp32 biases of (q|k|v, o, gate|up, down), None where a projection has none; None: a model without biases, for which
        # nothing is allocated and every path launches what it launched before
        self.bias = biases if any(b is not None for t in biases for b in t) else None
        self.head_w = prep(lm.lm_head.weight)
        self.inter = cfg.intermediate_size
        # LoRA adapters (train.LoraLinear on q / k / v), UNMERGED: per layer the (col0, A, B, scaling) segments of the fused q|k|v output that
        # ops.lora_update (vtgb_llm_lora) and ``_layer`` add after the base projection -- references to the model's own fp32 parameters, so the
        # base stream stays the packed weights above (bf16, or the quantised modes' dequantised values).  None: no adapters, nothing below changes.
        self.lora = None
        if has_lora:
            col0 = dict(q_proj=0, k_proj=self.nh * self.hd, v_proj=(self.nh + self.nkv) * self.hd)
            self.lora = [[(col0[p], m.lora_A["default"].weight.detach(), m.lora_B["default"].weight.detach(), float(m.scaling))
                          for p in _LORA_PROJECTIONS for m in (getattr(l.self_attn, p),) if hasattr(m, "lora_A")] for l in lm.model.layers]
        self._skinny = None           # per layer (wqkv, wo, wgu, wd) + lm_head in vtgb_gemm_skinny's tiled layout, built on first use

    # Projections of the decode step through libvtgb.so's own weight-streaming GEMM (vtgb_gemm_skinny, tiled weights), at every batch
    # it takes (one token per clip, <= 128 rows): no BLAS library call on the f2 path.  Measured on the Vicuna-7B shapes under hipGraph
    # replay (tools/exp/skinny_bench.py; profiles/r03_skinny_experiments.md): 4.7 vs 4.5 ms per token at batch 124, 4.0 vs 4.2 at batch 1
    # (hipBLASLt = F.linear).  Larger batches fall back to F.linear.
    SKINNY_MAX_BATCH = 128

    def _skinny_weights(self):
        if self._skinny is None:
            # (fp8: re-quantising the dequantised weights gives the same q * scale -- a row whose largest code rounded down to 224 comes back
            # as twice the codes under half the scale, the same numbers; mxfp4: a block's largest element dequantises to 4 or 6 times 2^e, which
            # gives the same e, the same codes and the same numbers -- ops.quantize_mxfp4_rows)
            pack = {"bf16": ops.SkinnyWeight, "fp8": ops.SkinnyWeightFp8, "mxfp4": ops.SkinnyWeightMxfp4}[self.weights]
            self._skinny = [tuple(pack(w) for w in (wqkv, wo, wgu, wd)) for (_, wqkv, wo, _, wgu, wd) in self.layers]
            self._skinny.append(pack(self.head_w))
        return self._skinny

    def _lora_of(self, li: int):
        return self.lora[li] if self.lora is not None else ()

    def _bias_of(self, li: int):
        """The layer's fp32 biases of (q|k|v, o, gate|up, down), None where there is none."""
        return self.bias[li] if self.bias is not None else (None, None, None, None)

    def _use_skinny(self, B: int, dtype) -> bool:
        H, I = self.cfg.hidden_size, self.inter
        return self.fused and dtype == torch.bfloat16 and B <= self.SKINNY_MAX_BATCH and H % 64 == 0 and I % 64 == 0 and (self.nh * self.hd) % 64 == 0

    def _rope(self, tmax: int, device, dtype):
        """cos / sin [tmax, hd] of rotary rows 0 .. tmax-1, operands of every consumer (append, prefill, beam tables).  A scaled type: the
        model's frequencies and factor, as LlamaRotaryEmbedding.forward -- (emb.cos() * attention_scaling).to(dtype)."""
        if self.rope_scaled is not None:
            inv, factor = self.rope_scaled
            fr = torch.arange(tmax, device=device, dtype=torch.float32)[:, None] * inv.to(device)[None]
            emb = torch.cat((fr, fr), dim=-1)
            return (emb.cos() * factor).to(dtype), (emb.sin() * factor).to(dtype)
        inv = 1.0 / (self.theta ** (torch.arange(0, self.hd, 2, device=device, dtype=torch.float32) / self.hd))
        fr = torch.arange(tmax, device=device, dtype=torch.float32)[:, None] * inv[None]
        emb = torch.cat((fr, fr), dim=-1)
        return emb.cos().to(dtype), emb.sin().to(dtype)

    def _layer(self, x, w, cos, sin, kc, vc, pos_idx, mask, codes=None, lora=(), bias=(None, None, None, None)):
        """x [B, S, H]; cos/sin [S, hd] (padded batches: [B, 1, S, hd], per-row positions); kc/vc [B, nkv, Tmax, hd]; pos_idx [S] cache rows
        to write; mask additive, broadcast to [B, 1, S, Tmax].  kv_cache="fp8": k and v pass through dq(q(.)) before the cache write and
        the attention -- the kernel-independent statement of the model.  ``codes`` = (kc8, vc8, ks, vs) of an fp8 state (prefill only,
        pos_idx = 0 .. S-1; kc / vc None): codes and scales go to the cache and the attention runs over the prompt's own dequantised K/V.
        ``lora``: the layer's adapter segments (``self.lora[li]``), added to q|k|v as train.LoraLinear.forward adds them -- behind the base
        projection's bias.  ``bias``: the layer's biases (``_bias_of``), F.linear's in the model's dtype."""
        ln1, wqkv, wo, ln2, wgu, wd = w
        bqkv, bo, bgu, bd = (None if b is None else b.to(x.dtype) for b in bias)
        B, S, _ = x.shape
        nq, nkv, hd = self.nh, self.nkv, self.hd
        h = _rms(x, ln1, self.eps)
        qkv = F.linear(h, wqkv, bqkv)
        for c0, la, lb, scaling in lora:      # result + (lora_B(lora_A(x.float())) * scaling).to(result.dtype), per adapted projection
            n = lb.shape[0]
            qkv = torch.cat((qkv[..., :c0], qkv[..., c0: c0 + n] + (F.linear(F.linear(h.to(la.dtype), la), lb) * scaling).to(qkv.dtype),
                             qkv[..., c0 + n:]), dim=-1)
        qkv = qkv.view(B, S, nq + 2 * nkv, hd).transpose(1, 2)      # [B, heads, S, hd]
        qk = qkv[:, : nq + nkv]
        qk = qk * cos + _rot_half(qk) * sin                                        # rotary on q and k together
        q, k, v = qk[:, :nq], qk[:, nq:], qkv[:, nq + nkv:]
        if codes is not None:
            kc8, vc8, ks, vs = codes
            (qk8, sk), (qv8, sv) = ops.quantize_fp8_kv(k), ops.quantize_fp8_kv(v)
            kc8.index_copy_(2, pos_idx, qk8.view(torch.uint8))
            vc8.index_copy_(2, pos_idx, qv8.view(torch.uint8))
            ks.index_copy_(2, pos_idx, sk)
            vs.index_copy_(2, pos_idx, sv)
            kk, vv = ops.dequantize_fp8_kv(qk8, sk, k.dtype), ops.dequantize_fp8_kv(qv8, sv, v.dtype)
            mask = mask[..., :S]
        else:
            if self.kv_cache == "fp8":
                k, v = ops.fp8_kv_round(k), ops.fp8_kv_round(v)
            kc.index_copy_(2, pos_idx, k)
            vc.index_copy_(2, pos_idx, v)
            kk, vv = kc, vc
        if nkv != nq:
            rep = nq // nkv
            kk, vv = kk.repeat_interleave(rep, 1), vv.repeat_interleave(rep, 1)
        a = F.scaled_dot_product_attention(q, kk, vv, attn_mask=mask)
        x = x + F.linear(a.transpose(1, 2).reshape(B, S, nq * hd), wo, bo)
        h = _rms(x, ln2, self.eps)
        gu = F.linear(h, wgu, bgu)
        return x + F.linear(F.silu(gu[..., : self.inter]) * gu[..., self.inter:], wd, bd)

    # Prefill on libvtgb.so: the four projections of a layer through vtgb_gemm (bf16: the persistent MFMA kernel, M = B*P rows; fp32:
    # the FMA kernel), the causal attention through ops.attention (bf16: vtgb_attention with the whole K/V of a head in LDS up to 288
    # tokens of equal head counts -- head_dim <= 128 --, vtgb_attention_tiled for longer prompts and grouped-query heads -- head_dim 64 /
    # 128, K / V heads read in place; fp32: the exactness kernel), RMSNorm(+residual), rotary + cache fill and SwiGLU through the
    # vtgb_llm_* kernels of the decode step -- no BLAS library call is left on the f2 path, in either dtype (round 4: the fp32 mode, whose
    # ids are compared token for token with HF generate, runs on libvtgb.so too; there grouped-query models repeat K / V heads).
    # Longer bf16 prompts are prefilled in chunks over the cache (_prefill_chunked below); PREFILL_MAX_TOKENS = 0 forces the torch path.  (The bound is the prefill's alone: the decode step's cache is P + max_new_tokens slots
    # rounded up to 64, and which attention kernel serves it is decided by DECODE_SPLIT_MIN_KEYS below.)  Activation memory of the bf16 path: B * P x intermediate_size bf16 (+ twice that for
    # gate | up) -- 0.72 GB (+ 1.44 GB) at B = 16, P = 2048 of Vicuna-7B.
    PREFILL_MAX_TOKENS = 2048
    PREFILL_MAX_TOKENS_F32 = 1024

    def _use_hip_prefill(self, x: Tensor, P: int) -> bool:
        if not (self.fused and x.is_cuda):
            return False
        if x.dtype == torch.float32:
            return P <= self.PREFILL_MAX_TOKENS_F32 and self.hd % 2 == 0 and self.hd <= 128
        if not (x.dtype == torch.bfloat16 and P <= self.PREFILL_MAX_TOKENS and self.cfg.hidden_size % 64 == 0 and self.inter % 64 == 0):
            return False
        if self.nq_eq_nkv and P <= 288:      # every head_dim the single-pass kernel takes at 288 keys (its bound at head_dim 96 and 128)
            return self.hd % 16 == 0 and self.hd <= 128
        # grouped heads or a longer prompt: ops.attention picks the kernel -- the tiled one, or still the single-pass one for equal
        # heads of head_dim 64 up to its 512 keys (ops._SINGLE_PASS_KEYS)
        return self.hd in ops._SINGLE_PASS_KEYS and self.nh % self.nkv == 0

    @property
    def nq_eq_nkv(self) -> bool:
        return self.nh == self.nkv

    def _prefill_hip(self, st, x: Tensor, P: int, pos_ids: Optional[Tensor] = None, key_mask: Optional[Tensor] = None) -> Tensor:
        """x [B, P, H] bf16 -> hidden state of the last position [B, H]; fills rows 0..P-1 of every layer's KV cache.  Padded batches:
        ``pos_ids`` [B, P] (the rotary rows) and ``key_mask`` [B, P] fp32 (0 / finfo(float32).min: pad keys get no weight; a query with
        no valid key -- a leading pad -- stays finite)."""
        lib, stream, code = L.lib(), _stream(), dtype_code(x.dtype)
        B, _, H = x.shape
        nh, nkv, hd, M = self.nh, self.nkv, self.hd, B * P
        x = x.reshape(M, H).clone()
        h = torch.empty_like(x)
        act = torch.empty(M, self.inter, dtype=x.dtype, device=x.device)
        delta = None
        for li, (ln1, wqkv, wo, ln2, wgu, wd) in enumerate(self.layers):
            bqkv, bo, bgu, bd = self._bias_of(li)
            L.check(lib.vtgb_llm_rmsnorm(code, _ptr(x), _ptr(delta), _ptr(ln1), _ptr(h), M, H, self.eps, stream))
            qkv = ops.gemm(h, wqkv, bias=bqkv)
            if self.lora is not None and self.lora[li]:      # the adapters act on q|k|v before rotary and before K/V are quantised, as in the model
                ops.lora_update(h, qkv, self.lora[li])
            qkv = qkv.view(B, P, nh + 2 * nkv, hd)
            # rotary on q and k in place + k / v into the cache rows 0 .. P-1: one launch (HF's roundings in the model's dtype)
            if st["attn"] == "split_fp8":      # codes + scales into the cache, the dequantised k / v back into qkv for the attention below
                L.check(lib.vtgb_llm_rope_cache_prefill_fp8(code, _ptr(qkv), _ptr(st["kc8"][li]), _ptr(st["vc8"][li]), _ptr(st["ks"][li]),
                                                            _ptr(st["vs"][li]), _ptr(st["cos"]), _ptr(st["sin"]), _ptr(pos_ids), B, P, nh, nkv, hd,
                                                            st["tmax"], stream))
            else:
                cache = (_ptr(qkv), _ptr(st["kc"][li]), _ptr(st["vc"][li]), _ptr(st["cos"]), _ptr(st["sin"]))
                if pos_ids is None:
                    L.check(lib.vtgb_llm_rope_cache_prefill(code, *cache, B, P, nh, nkv, hd, st["tmax"], stream))
                else:
                    L.check(lib.vtgb_llm_rope_cache_prefill_pos(code, *cache, _ptr(pos_ids), B, P, nh, nkv, hd, st["tmax"], stream))
            flat = qkv.view(B, P, (nh + 2 * nkv) * hd)
            q_, k_, v_ = flat[:, :, : nh * hd], flat[:, :, nh * hd: (nh + nkv) * hd], flat[:, :, (nh + nkv) * hd:]
            if nkv != nh and x.dtype != torch.bfloat16:      # fp32, grouped-query attention: every K / V head serves nh / nkv query heads (a copy; bf16 reads them in place)
                rep = nh // nkv
                k_ = k_.reshape(B, P, nkv, 1, hd).expand(B, P, nkv, rep, hd).reshape(B, P, nh * hd)
                v_ = v_.reshape(B, P, nkv, 1, hd).expand(B, P, nkv, rep, hd).reshape(B, P, nh * hd)
            a = ops.attention(q_, k_, v_, nh, float(hd) ** -0.5, key_mask=key_mask, causal=True, kv_heads=nkv if x.dtype == torch.bfloat16 else None)
            o = ops.gemm(a.view(M, nh * hd), wo, bias=bo)
            L.check(lib.vtgb_llm_rmsnorm(code, _ptr(x), _ptr(o), _ptr(ln2), _ptr(h), M, H, self.eps, stream))
            gu = ops.gemm(h, wgu, bias=bgu)
            L.check(lib.vtgb_llm_silu_mul(code, _ptr(gu), _ptr(act), M, self.inter, stream))
            delta = ops.gemm(act, wd, bias=bd)
        return x.view(B, P, H)[:, -1] + delta.view(B, P, H)[:, -1]

    # Chunked prefill: a bf16 prompt past PREFILL_MAX_TOKENS goes through the layer stack in chunks of at most PREFILL_CHUNK_TOKENS rows, one
    # after the other; every chunk appends its K / V to the cache and attends over the cache -- everything before it plus itself
    # (ops.attention_cached: vtgb_attention_cached, caches up to 16384 slots, bf16 or the fp8 codes).  Activation memory is one chunk's
    # (B * 2048 rows), whatever P.  Prompts up to PREFILL_MAX_TOKENS keep the one-shot sequence above and its bits.
    PREFILL_CHUNK_TOKENS = 2048

    def _use_chunked_prefill(self, st, x: Tensor, P: int) -> bool:
        """Whether ``_prefill_chunked`` takes the prompt: the one-shot prefill refuses it for its length alone, and the state's cache is one
        vtgb_attention_cached reads (bf16, or the fp8 code caches; up to 16384 slots).  PREFILL_MAX_TOKENS = 0 still forces the torch path."""
        if not (self.fused and x.is_cuda and x.dtype == torch.bfloat16):
            return False
        if not (0 < self.PREFILL_MAX_TOKENS < P and self.PREFILL_CHUNK_TOKENS > 0):
            return False
        if not (self.hd in (64, 128) and self.nh % self.nkv == 0 and self.cfg.hidden_size % 64 == 0 and self.inter % 64 == 0):
            return False
        if st["tmax"] > ops.ATTENTION_CACHED_MAX_KEYS:
            return False
        return st["attn"] == "split_fp8" or (self.kv_cache == "bf16" and "kc" in st)

    def _prefill_chunked(self, st, x: Tensor, P: int, pos_ids: Optional[Tensor] = None) -> Tensor:
        """``_prefill_hip`` in chunks (``prefill_chunks(P, PREFILL_CHUNK_TOKENS)``): x [B, P, H] bf16 -> hidden state of the last position
        [B, H]; fills rows 0..P-1 of every layer's KV cache.  Per chunk [q0, q0 + n) and layer the launches are ``_prefill_hip``'s, except
        that rotary + append write cache rows q0 .. q0+n-1 with the rotary rows q0 + s (padded: ``pos_ids[:, q0:q0+n]``) -- the same
        entries, which address the cache and the tables only through base pointers and (b, head, row) strides, given pointers advanced by
        q0 rows -- and that the attention reads K / V from the cache the append just wrote (padded: the state's ``key_valid``)."""
        lib, stream, code = L.lib(), _stream(), dtype_code(x.dtype)
        B, _, H = x.shape
        nh, nkv, hd, tmax = self.nh, self.nkv, self.hd, st["tmax"]
        fp8 = st["attn"] == "split_fp8"
        key_valid = st.get("key_valid")
        scale = float(hd) ** -0.5
        last = None
        for q0, n in prefill_chunks(P, self.PREFILL_CHUNK_TOKENS):
            M = B * n
            xc = x[:, q0: q0 + n].reshape(M, H).clone()
            h = torch.empty_like(xc)
            act = torch.empty(M, self.inter, dtype=x.dtype, device=x.device)
            pid = None if pos_ids is None else pos_ids[:, q0: q0 + n].contiguous()
            # (the rotary row is the table's row s without pos_ids -- tables advanced by q0 rows -- and pos_ids[b, s] with them: tables as they are)
            cos, sin = (st["cos"], st["sin"]) if pid is not None else (st["cos"][q0:], st["sin"][q0:])
            delta = None
            for li, (ln1, wqkv, wo, ln2, wgu, wd) in enumerate(self.layers):
                bqkv, bo, bgu, bd = self._bias_of(li)
                L.check(lib.vtgb_llm_rmsnorm(code, _ptr(xc), _ptr(delta), _ptr(ln1), _ptr(h), M, H, self.eps, stream))
                qkv = ops.gemm(h, wqkv, bias=bqkv)
                if self.lora is not None and self.lora[li]:
                    ops.lora_update(h, qkv, self.lora[li])
                qkv = qkv.view(B, n, (nh + 2 * nkv) * hd)
                if fp8:      # (the entry also writes the dequantised k / v back into qkv: unused here, K / V have one source, the cache)
                    kc, vc, sc = st["kc8"][li], st["vc8"][li], (st["ks"][li], st["vs"][li])
                    L.check(lib.vtgb_llm_rope_cache_prefill_fp8(code, _ptr(qkv), _ptr(kc[:, :, q0:]), _ptr(vc[:, :, q0:]), _ptr(sc[0][:, :, q0:]),
                                                                _ptr(sc[1][:, :, q0:]), _ptr(cos), _ptr(sin), _ptr(pid), B, n, nh, nkv, hd, tmax, stream))
                else:
                    kc, vc, sc = st["kc"][li], st["vc"][li], None
                    cache = (_ptr(qkv), _ptr(kc[:, :, q0:]), _ptr(vc[:, :, q0:]), _ptr(cos), _ptr(sin))
                    if pid is None:
                        L.check(lib.vtgb_llm_rope_cache_prefill(code, *cache, B, n, nh, nkv, hd, tmax, stream))
                    else:
                        L.check(lib.vtgb_llm_rope_cache_prefill_pos(code, *cache, _ptr(pid), B, n, nh, nkv, hd, tmax, stream))
                a = ops.attention_cached(qkv[:, :, : nh * hd], kc, vc, q0, nh, scale, key_valid=key_valid, scales=sc)
                o = ops.gemm(a.view(M, nh * hd), wo, bias=bo)
                L.check(lib.vtgb_llm_rmsnorm(code, _ptr(xc), _ptr(o), _ptr(ln2), _ptr(h), M, H, self.eps, stream))
                gu = ops.gemm(h, wgu, bias=bgu)
                L.check(lib.vtgb_llm_silu_mul(code, _ptr(gu), _ptr(act), M, self.inter, stream))
                delta = ops.gemm(act, wd, bias=bd)
            last = xc.view(B, n, H)[:, -1] + delta.view(B, n, H)[:, -1]
        return last

    def _head(self, x):
        h = _rms(x, self.lm.model.norm.weight, self.eps)
        if h.is_cuda and h.dim() == 2 and self._use_skinny(h.shape[0], h.dtype):
            return ops.gemm_skinny(h.contiguous(), self._skinny_weights()[-1])      # the first token's logits: same kernel as the decode step's
        if h.is_cuda and h.dim() == 2 and self.fused and h.dtype in (torch.float32, torch.bfloat16) and self._gemm_ok(h.dtype):
            return ops.gemm(h.contiguous(), self.head_w)                            # fp32 (exactness mode) / batches beyond the skinny kernel: vtgb_gemm
        return F.linear(h, self.head_w)

    def _gemm_ok(self, dtype) -> bool:
        """vtgb_gemm takes these projections: any shape at fp32; bf16 needs 8-aligned rows."""
        return dtype == torch.float32 or (self.cfg.hidden_size % 8 == 0 and self.inter % 8 == 0 and (self.nh * self.hd) % 8 == 0)

    # Decode attention: caches of DECODE_SPLIT_MIN_KEYS slots and more (head_dim 64 / 128, up to 16384 slots) run on the split-KV kernel
    # (vtgb_llm_decode_attention_split: 256-key chunks over workgroups, K/V read once per group of query heads), shorter ones on the
    # one-wave-per-head kernel, which ends at 2048 slots.  The value (2112) is the routing rule's fallback -- the split kernel only where the
    # other refuses -- until the two kernels are timed against each other ("Split-KV decode attention"); from a lower
    # value upward bf16 ids may differ from the other kernel's where two logits tie within a rounding (another summation order).  A cache
    # neither kernel takes (more than 2048 slots at another head_dim, or more than 16384) decodes on the torch step.  The kernel is picked
    # once per state, when its buffers are built (st["attn"]: "split", "single" or None), and the step follows the state.
    DECODE_SPLIT_MIN_KEYS = ops.DECODE_SPLIT_MIN_KEYS

    def _attn_route(self, tmax: int) -> Optional[str]:
        return ops.decode_attention_route(tmax, self.hd, self.DECODE_SPLIT_MIN_KEYS)

    def _state(self, B: int, P: int, N: int, device, dtype, eos=None, pad=0, min_new=0, sample=None, stop=None, padded=False, penalty: float = 1.0):
        # The cache length is bucketed (multiples of 64) and the true prompt length is device data (`pos`): an eval loop over real
        # questions with varying P reuses a handful of graphs instead of capturing one -- and allocating 2 x n_layers KV caches --
        # per distinct P.  At most MAX_STATES states are kept (least recently used goes: graph and caches are freed).  A padded batch has
        # states of its own, whose per-row key mask and rotary offsets are device buffers written before every call: ragged batches of one
        # shape share one graph.  Padded and unpadded states share the MAX_STATES slots, so a loop that alternates both over more than
        # MAX_STATES (batch, bucket, settings) combinations captures graphs again where an unpadded-only loop would not.
        tmax = -(-(P + N) // 64) * 64
        H, HD, inter = self.cfg.hidden_size, self.nh * self.hd, self.inter

        def z(*shape, dtype=dtype):
            return torch.zeros(*shape, device=device, dtype=dtype)

        def buffers():
            cos, sin = self._rope(tmax, device, dtype)
            attn = self._attn_route(tmax) if device.type == "cuda" and self.fused else None
            if self.kv_cache == "fp8":      # the code caches where the fp8 split kernel serves the state, else bf16 caches of dequantised values + the torch step
                attn = "split_fp8" if (attn is not None and dtype == torch.bfloat16 and ops.decode_attention_fp8_ok(tmax, self.hd)
                                       and self.nh % self.nkv == 0) else None
            st = dict(cos=cos, sin=sin, tmax=tmax, attn=attn, x=z(B, H), h=z(B, H), q=z(B, HD), a=z(B, HD), act=z(B, inter))
            if attn == "split_fp8":
                st.update(kc8=[z(B, self.nkv, tmax, self.hd, dtype=torch.uint8) for _ in self.layers],
                          vc8=[z(B, self.nkv, tmax, self.hd, dtype=torch.uint8) for _ in self.layers],
                          ks=[z(B, self.nkv, tmax, dtype=torch.float32) for _ in self.layers],
                          vs=[z(B, self.nkv, tmax, dtype=torch.float32) for _ in self.layers])
            else:
                st.update(kc=[z(B, self.nkv, tmax, self.hd) for _ in self.layers], vc=[z(B, self.nkv, tmax, self.hd) for _ in self.layers])
            if padded:      # key_valid[b, t]: cache slot t holds a real key of row b; rope_off[b]: rotary row - cache row of its decode steps
                st.update(key_valid=torch.ones(B, tmax, dtype=torch.uint8, device=device), rope_off=z(B, dtype=torch.long))
            if attn in ("split", "split_fp8"):      # the split kernel's per-chunk partials
                st.update(attn_ws=z(ops.decode_attention_workspace_bytes(B, self.nh, self.hd, tmax), dtype=torch.uint8))
            if device.type == "cuda" and self._use_skinny(B, dtype):
                Hq, V = (self.nh + 2 * self.nkv) * self.hd, self.head_w.shape[0]
                shapes = ((Hq, H), (H, HD), (2 * inter, H), (H, inter), (V, H))
                st.update(sk_qkv=z(B, Hq), sk_o=z(B, H), sk_gu=z(B, 2 * inter), sk_d=z(B, H), sk_logits=z(B, V),
                          sk_ws=z(max(ops.gemm_skinny_workspace_bytes(B, n, k) for n, k in shapes), dtype=torch.uint8))
                self._skinny_weights()
            return st
        key = (B, tmax, N, eos, pad, min_new, sample, stop, padded) + ((self.kv_cache,) if self.kv_cache != "bf16" else ())
        return self._cached_state(key, B, N, tmax, device, eos, pad, min_new, sample, stop, buffers, penalty)

    def _decode_step_fused(self, st):
        """One token for every sequence with the per-layer small ops fused in libvtgb.so
        (include/vtgb.h vtgb_llm_*): per layer 4 GEMMs + 5 fused launches instead of ~25."""
        lib, stream = L.lib(), _stream()
        x = st["x"]
        x.copy_(self.lm.get_input_embeddings()(st["tok"]))
        B, H = x.shape
        code = dtype_code(x.dtype)
        nq, nkv, hd, tmax = self.nh, self.nkv, self.hd, st["tmax"]
        padded, skinny = "key_valid" in st, "sk_ws" in st
        # a beam state (st["attn"] == "beam"): the rows are the B * K beams; a row appends its K/V at slot = the step of the generated caches
        # kg / vg (rotary row = slot + rope_off[r] of the state's tables) and attends through the ancestry table over the prompt cache of its
        # batch item (B rows: the key mask is the batch item's) and the generated caches (vtgb_llm_decode_attention_beam)
        # ("beam_fp8": the same over fp8 caches -- kg8 / vg8 / kgs / vgs, a prompt state of code caches, vtgb_llm_decode_attention_beam_fp8)
        beam_fp8 = st["attn"] == "beam_fp8"
        beam = st["attn"] == "beam" or beam_fp8
        row_off = padded or beam
        h, q, a, act = st["h"], st["q"], st["a"], st["act"]
        if skinny:
            sw, ws = self._skinny_weights(), st["sk_ws"]

            def lin(xin, li, which, buf):      # which: 0 qkv, 1 o, 2 gate|up, 3 down
                return ops.gemm_skinny(xin, sw[li][which], out=st[buf], workspace=ws, bias=self._bias_of(li)[which])
        elif self._gemm_ok(x.dtype):
            def lin(xin, li, which, buf):      # fp32 (exactness mode) and batches beyond the skinny kernel: libvtgb.so's own GEMM, no BLAS
                return ops.gemm(xin, self.layers[li][(1, 2, 4, 5)[which]], bias=self._bias_of(li)[which])
        else:
            def lin(xin, li, which, buf):
                b_ = self._bias_of(li)[which]
                return F.linear(xin, self.layers[li][(1, 2, 4, 5)[which]], None if b_ is None else b_.to(xin.dtype))
        # skinny path (bf16, batch <= 128): the split-K projections (qkv, o, down) leave their fp32 fragments in the workspace and the kernel that
        # consumes them (rotary + cache / RMSNorm + residual) adds them itself: 10 launches per layer instead of 13, the same values bit for bit
        defer = skinny and H in (2048, 4096)

        def lin_d(xin, li, which, buf):        # -> (tensor, n_splits): n_splits > 1 means "fragments in ws, tensor not written"
            if not defer:
                return lin(xin, li, which, buf), 1
            o_, S_, _ = ops.gemm_skinny(xin, sw[li][which], out=st[buf], workspace=ws, defer_reduce=True, bias=self._bias_of(li)[which])
            return o_, S_

        def norm(delta_t, delta_S, wt):
            if delta_t is not None and delta_S > 1:
                L.check(lib.vtgb_llm_rmsnorm_parts(code, _ptr(x), _ptr(ws), delta_S, _ptr(wt), _ptr(h), B, H, self.eps, stream))
            else:
                L.check(lib.vtgb_llm_rmsnorm(code, _ptr(x), _ptr(delta_t), _ptr(wt), _ptr(h), B, H, self.eps, stream))
        # rotary + cache append: vtgb_llm_rope_cache{,_parts}{,_pos} (_parts: q|k|v arrive as split-K fragments; _pos: a padded batch's per-row
        # rotary offsets) take the same pointer lists apart from those extras.  Attention: ops.decode_attention, the kernel fixed by the state
        # (its workspace exists exactly where the split kernel serves it)
        rope = (_ptr(st["cos"]), _ptr(st["sin"]), _ptr(st["slot"] if beam else st["pos"])) + ((_ptr(st["rope_off"]),) if row_off else ())
        attn_ws, key_valid = st.get("attn_ws"), st.get("key_valid")
        fp8_kv = st["attn"] == "split_fp8" or beam_fp8      # kv_cache="fp8": the append quantises the K / V rows, the attention reads codes and scales
        delta, dS = None, 1
        for li, (ln1, wqkv, wo, ln2, wgu, wd) in enumerate(self.layers):
            norm(delta, dS, ln1)
            if self.lora is not None and self.lora[li]:      # adapters: q|k|v materialised (this one projection is not deferred), updated in place
                qkv, qS = ops.lora_update(h, lin(h, li, 0, "sk_qkv"), self.lora[li]), 1
            else:
                qkv, qS = lin_d(h, li, 0, "sk_qkv")
            if fp8_kv:
                kv8 = tuple(st[n][li] for n in (("kg8", "vg8", "kgs", "vgs") if beam else ("kc8", "vc8", "ks", "vs")))
                ra = L.LlmRopeCacheFp8Args(code, B, nq, nkv, hd, st["tmax_g"] if beam else tmax, qS if qS > 1 else 0, None if qS > 1 else _ptr(qkv),
                                           _ptr(ws) if qS > 1 else None, _ptr(q), *(_ptr(t) for t in kv8), *rope[:3], rope[3] if row_off else None)
                L.check(lib.vtgb_llm_rope_cache_fp8(ctypes.byref(ra), stream))
                if beam:
                    pst = st["prompt"]
                    ops.decode_attention_beam_fp8(q, pst["kc8"][li], pst["vc8"][li], pst["ks"][li], pst["vs"][li], *kv8, st["src_row"], st["nprompt"],
                                                  st["pos"], float(hd) ** -0.5, key_valid=key_valid, out=a, workspace=attn_ws)
                else:
                    ops.decode_attention_fp8(q, *kv8, st["pos"], float(hd) ** -0.5, key_valid=key_valid, out=a, workspace=attn_ws)
            else:
                kc, vc = (st["kg"][li], st["vg"][li]) if beam else (st["kc"][li], st["vc"][li])
                rope_cache = getattr(lib, "vtgb_llm_rope_cache" + ("_parts" if qS > 1 else "") + ("_pos" if row_off else ""))
                L.check(rope_cache(code, *((_ptr(ws), qS) if qS > 1 else (_ptr(qkv),)), _ptr(q), _ptr(kc), _ptr(vc), *rope, B, nq, nkv, hd,
                                   st["tmax_g"] if beam else tmax, stream))
                if beam:
                    ops.decode_attention_beam(q, st["prompt"]["kc"][li], st["prompt"]["vc"][li], kc, vc, st["src_row"], st["nprompt"], st["pos"],
                                              float(hd) ** -0.5, key_valid=key_valid, out=a, workspace=attn_ws)
                else:
                    ops.decode_attention(q, kc, vc, st["pos"], float(hd) ** -0.5, key_valid=key_valid, out=a, workspace=attn_ws,
                                         split=st["attn"] == "split")
            o, oS = lin_d(a, li, 1, "sk_o")
            norm(o, oS, ln2)
            gu = lin(h, li, 2, "sk_gu")
            L.check(lib.vtgb_llm_silu_mul(code, _ptr(gu), _ptr(act), B, self.inter, stream))
            delta, dS = lin_d(act, li, 3, "sk_d")
        norm(delta, dS, self.lm.model.norm.weight)
        emit = self._beam_emit if beam else self._emit
        if skinny:
            emit(st, ops.gemm_skinny(h, sw[-1], out=st["sk_logits"], workspace=ws))
        elif self._gemm_ok(x.dtype):
            emit(st, ops.gemm(h, self.head_w))
        else:
            emit(st, F.linear(h, self.head_w))

    def _decode_step(self, st):
        """One token for every sequence, entirely on the device (captured)."""
        if st["attn"] is not None:      # fused, on the device, and a kernel takes the cache
            return self._decode_step_fused(st)
        emb = self.lm.get_input_embeddings()
        x = emb(st["tok"])[:, None, :]
        pos = st["pos"]
        neg = torch.finfo(x.dtype).min
        if "key_valid" in st:      # padded: rotary row pos + rope_off[b], pad keys masked
            rp = pos + st["rope_off"]
            cos, sin = st["cos"].index_select(0, rp)[:, None, None, :], st["sin"].index_select(0, rp)[:, None, None, :]
            ok = (st["ar"][None, :] <= pos) & (st["key_valid"] != 0)
            mask = torch.where(ok, 0.0, neg).to(x.dtype)[:, None, None, :]
        else:
            cos, sin = st["cos"].index_select(0, pos), st["sin"].index_select(0, pos)
            mask = torch.where(st["ar"][None, None, None, :] <= pos, 0.0, neg).to(x.dtype)
        for li, w in enumerate(self.layers):
            x = self._layer(x, w, cos, sin, st["kc"][li], st["vc"][li], pos, mask, lora=self._lora_of(li), bias=self._bias_of(li))
        (self._beam_emit if "beam" in st else self._emit)(st, self._head(x[:, -1]))

    # ---- beam search (opt-in at the interfaces: beam_search="graph").  R = B * K rows run the decode step.  On the device (fused) the state keeps
    # the prompt's K/V once per batch item (``st["prompt"]``: a B-row state the prefill entries fill, unchanged) and what the beams generate in
    # kg / vg [R, nkv, tmax_g, hd], one slot per step; re-ordering beams re-orders an int32 ancestry table (``src_row``), never K/V, and the
    # attention reads through it (vtgb_llm_decode_attention_beam, whatever the cache length).  The append is the existing
    # vtgb_llm_rope_cache{,_parts}_pos entry on the generated caches: cache row = slot, rotary row = slot + rope_off[r] of tables that are
    # written before every call to start at the batch's first generated position (cos / sin [tmax_g, hd]; tmax_g covers N plus the spread of
    # the rows' first positions in a ragged batch).  Elsewhere (CPU, fused=False) the rows keep whole caches, re-ordered by index_select as
    # HF re-orders its cache: the torch statement of the same search.
    # kv_cache="fp8" under ``fp8_beams``: on the device the prompt state is an fp8 prefill state (attn "split_fp8": kc8 / vc8 / ks / vs on B rows)
    # and the generated caches are kg8 / vg8 [R, nkv, tmax_g, hd] uint8 with kgs / vgs [R, nkv, tmax_g] fp32 (attn "beam_fp8":
    # vtgb_llm_rope_cache_fp8 appends, vtgb_llm_decode_attention_beam_fp8 reads); elsewhere ``_layer`` rounds K/V into the whole caches.
    def _beam_state(self, B: int, K: int, P: int, N: int, device, dtype, eos, fill: int, min_new: int, rep_pen: float, len_pen: float, padded: bool,
                    spread: int):
        R = B * K
        kernel = device.type == "cuda" and self.fused
        H, HD, inter, nkv, hd = self.cfg.hidden_size, self.nh * self.hd, self.inter, self.nkv, self.hd
        tmax_p, tmax_g = -(-P // 64) * 64, -(-(N + spread) // 64) * 64
        if not kernel:
            tmax_p, tmax_g = -(-(P + N) // 64) * 64, 0      # (one cache per row, as the plain decoder's)
        elif not ((ops.decode_attention_beam_fp8_ok if self.kv_cache == "fp8" else ops.decode_attention_beam_ok)(tmax_p, tmax_g, hd) and self.nh % nkv == 0):
            raise NotImplementedError(f"num_beams > 1 on the device needs head_dim 64 or 128 and a cache up to {ops.DECODE_SPLIT_MAX_KEYS} slots "
                                      f"(head_dim {hd}, {tmax_p} + {tmax_g} slots)")
        elif K > ops.BEAM_MAX_BEAMS or 2 * K > self.head_w.shape[0]:
            raise NotImplementedError(f"num_beams={K}: up to {ops.BEAM_MAX_BEAMS} beams, 2 x num_beams <= vocab_size")
        tmax = tmax_p + tmax_g
        fp8 = kernel and self.kv_cache == "fp8"      # the code caches (the fused device path takes a bf16 model: the constructor); elsewhere ``_layer`` rounds

        def z(*shape, dtype=dtype):
            return torch.zeros(*shape, device=device, dtype=dtype)

        def caches(rows, slots):      # per layer: codes, codes, scales, scales (fp8) or K, V
            def per_layer(*tail, dtype=dtype):
                return [z(rows, nkv, slots, *tail, dtype=dtype) for _ in self.layers]
            if fp8:
                return (per_layer(hd, dtype=torch.uint8), per_layer(hd, dtype=torch.uint8), per_layer(dtype=torch.float32), per_layer(dtype=torch.float32))
            return per_layer(hd), per_layer(hd)

        def buffers():
            cos, sin = self._rope(tmax, device, dtype)
            pst = dict(ar=torch.arange(tmax_p, device=device), cos=cos[:tmax_p], sin=sin[:tmax_p], tmax=tmax_p,
                       attn=("split_fp8" if fp8 else "split") if kernel else None)
            pst.update(zip(("kc8", "vc8", "ks", "vs") if fp8 else ("kc", "vc"), caches(B, tmax_p)))
            if padded:
                pst.update(key_valid=torch.ones(B, tmax_p, dtype=torch.uint8, device=device), rope_off=z(B, dtype=torch.long))
            st = dict(tmax=tmax, tmax_g=tmax_g, prompt=pst, attn=("beam_fp8" if fp8 else "beam") if kernel else None,
                      beam=dict(K=K, fill=fill, repetition_penalty=rep_pen, length_penalty=len_pen, kernel=kernel))
            st.update(self._beam_book(B, K, N, device, fill))
            if kernel:
                V = self.head_w.shape[0]
                st.update(zip(("kg8", "vg8", "kgs", "vgs") if fp8 else ("kg", "vg"), caches(R, tmax_g)))
                st.update(cos_full=cos, sin_full=sin, cos=z(tmax_g, hd), sin=z(tmax_g, hd), x=z(R, H), h=z(R, H), q=z(R, HD), a=z(R, HD), act=z(R, inter),
                          src_row=z(R, tmax_g, dtype=torch.int32), row_id=torch.arange(R, dtype=torch.int32, device=device)[:, None],
                          slot=z(1, dtype=torch.long), nprompt=z(1, dtype=torch.long), rope_off=z(R, dtype=torch.long),
                          attn_ws=z(ops.decode_attention_workspace_bytes(R, self.nh, hd, tmax), dtype=torch.uint8),
                          cand_ws=z(ops.beam_candidates_workspace_bytes(R, K, V), dtype=torch.uint8),
                          feedback=("tok", "pos", "step", "slot", "src_row") + self.BEAM_BOOK)
                if padded:
                    st["key_valid"] = pst["key_valid"]      # [B, tmax_p]: the batch item's prompt mask
                if self._use_skinny(R, dtype):
                    Hq = (self.nh + 2 * nkv) * hd
                    shapes = ((Hq, H), (H, HD), (2 * inter, H), (H, inter), (V, H))
                    st.update(sk_qkv=z(R, Hq), sk_o=z(R, H), sk_gu=z(R, 2 * inter), sk_d=z(R, H), sk_logits=z(R, V),
                              sk_ws=z(max(ops.gemm_skinny_workspace_bytes(R, n, k) for n, k in shapes), dtype=torch.uint8))
                    self._skinny_weights()
            else:
                st.update(cos=cos, sin=sin, kc=[z(R, nkv, tmax, hd) for _ in self.layers], vc=[z(R, nkv, tmax, hd) for _ in self.layers])
                if padded:
                    st.update(key_valid=torch.ones(R, tmax, dtype=torch.uint8, device=device), rope_off=z(R, dtype=torch.long))
            return st
        key = ("beams", B, K, tmax_p, tmax_g, N, eos, fill, min_new, rep_pen, len_pen, padded)
        return self._cached_state(key, R, N, tmax, device, eos, fill, min_new, None, None, buffers)

    def _beam_emit(self, st, logits: Tensor):
        """``_emit`` of a beam state: the selection, then the beams' K/V follow their parents -- the ancestry table on the device
        (src_row' = src_row[parent], and the slot the new tokens will be appended at is the row's own), whole caches elsewhere."""
        rows = self._beam_select(st, logits)
        if st["attn"] in ("beam", "beam_fp8"):
            st["src_row"].copy_(st["src_row"].index_select(0, rows))
            st["src_row"].index_copy_(1, st["step"], st["row_id"])
            st["slot"].add_(1)
        else:
            for c in st["kc"] + st["vc"]:
                c.copy_(c.index_select(0, rows))
        st["pos"].add_(1)
        st["step"].add_(1)

    def _generate_beams(self, inputs_embeds: Tensor, N: int, use_graph: bool, eos_token_id, pad_token_id, min_new_tokens, attention_mask, K: int,
                        length_penalty: float, repetition_penalty: float) -> Tensor:
        B, P, _ = inputs_embeds.shape
        pmask = _padding(attention_mask, B, P)
        dev, dt = inputs_embeds.device, inputs_embeds.dtype
        eos, _, min_new = self._special(eos_token_id, pad_token_id, min_new_tokens)
        fill = -1 if eos is None else int(pad_token_id if pad_token_id else _first_eos(eos))      # HF: ``pad_token_id or eos_token_id`` -- pad 0 fills with eos (a set: its first id)
        # the rotary row of every item's first generated token (HF: position_ids[b, P-1] + 1), from the host copy of the mask
        if pmask is None:
            first = torch.full((B,), P, dtype=torch.long)
        else:
            first = torch.where(pmask[:, -1] != 0, (pmask != 0).sum(-1), torch.ones(B, dtype=torch.long)).long()
        lo = int(first.min())
        st = self._beam_state(B, K, P, N, dev, dt, eos, fill, min_new, float(repetition_penalty), float(length_penalty), pmask is not None,
                              int(first.max()) - lo)
        pst = st["prompt"]
        logits = self._head(self._prefill(pst, inputs_embeds, pmask))      # [B, V]: the prompt runs once per batch item
        if st["attn"] in ("beam", "beam_fp8"):
            st["cos"].copy_(st["cos_full"][lo: lo + st["tmax_g"]])
            st["sin"].copy_(st["sin_full"][lo: lo + st["tmax_g"]])
            st["rope_off"].copy_((first - lo).repeat_interleave(K).to(dev))
            st["nprompt"].fill_(P)
            st["slot"].fill_(-1)
            st["src_row"].zero_()
        else:
            for src, dst in zip(pst["kc"] + pst["vc"], st["kc"] + st["vc"]):
                dst.copy_(src.repeat_interleave(K, 0))
            if pmask is not None:
                st["key_valid"].copy_(pst["key_valid"].repeat_interleave(K, 0))
                st["rope_off"].copy_(pst["rope_off"].repeat_interleave(K))
        self._beam_reset(st)
        st["step"].zero_()
        st["pos"].fill_(P - 1)
        self._beam_emit(st, logits.repeat_interleave(K, 0).contiguous())      # the first step: K identical rows, running scores [0, -1e9, ...]
        return self._replay_beams(st, use_graph)

    def _prefill(self, st, inputs_embeds: Tensor, pmask: Optional[Tensor]) -> Tensor:
        """The prompt through the layer stack into the state's K/V cache rows 0 .. P-1 (eager: a handful of large GEMMs); a padded batch's key mask
        and rotary offsets into the state's device buffers.  Returns the hidden state of the last position [B, H]."""
        B, P, _ = inputs_embeds.shape
        dev, dt = inputs_embeds.device, inputs_embeds.dtype
        x = inputs_embeds
        pidx = st["ar"][:P]
        pos_ids = key_mask = None
        if pmask is not None:        # (device buffers of the state, written outside any capture)
            valid = pmask.to(dev) != 0
            pos_ids = (valid.long().cumsum(-1) - 1).masked_fill(~valid, 0)                                # GenerationMixin._prepare_position_ids_for_generation
            st["key_valid"][:, :P].copy_(valid)
            st["key_valid"][:, P:].fill_(1)                                                               # generated keys
            st["rope_off"].copy_(pos_ids[:, P - 1] - (P - 1))                                             # _update_model_kwargs_for_generation: last + 1 per step
            key_mask = torch.where(valid, 0.0, torch.finfo(torch.float32).min).float().contiguous()      # [B, P] additive, vtgb_attention's

        def torch_operands():      # what ``_layer`` takes -- the additive mask is P x Tmax per row: built on the torch branches alone
            if pmask is None:
                causal = torch.where(st["ar"][None, :] <= pidx[:, None], 0.0, torch.finfo(dt).min).to(dt)[None, None]   # [1,1,P,Tmax]
                return st["cos"][:P], st["sin"][:P], causal
            ok = (st["ar"][None, :] <= pidx[:, None])[None] & (st["key_valid"][:, None, :] != 0)          # [B, P, Tmax]
            return (st["cos"][pos_ids][:, None], st["sin"][pos_ids][:, None],                             # [B, 1, P, hd]
                    torch.where(ok, 0.0, torch.finfo(dt).min).to(dt)[:, None])
        fp8_state = st["attn"] == "split_fp8"
        # (kv_cache="fp8" without the code caches -- the fallback state -- prefills on the torch path, which writes dequantised K/V)
        if self._use_hip_prefill(x, P) and (self.kv_cache == "bf16" or fp8_state):
            last = self._prefill_hip(st, x, P, pos_ids, key_mask)
        elif self._use_chunked_prefill(st, x, P):      # past the one-shot bound: chunks over the cache
            last = self._prefill_chunked(st, x, P, pos_ids)
        elif fp8_state:      # a prompt past the prefill kernels' bound into an fp8 state: quantised on the torch path
            cos, sin, causal = torch_operands()
            for li, w in enumerate(self.layers):
                x = self._layer(x, w, cos, sin, None, None, pidx, causal, codes=(st["kc8"][li], st["vc8"][li], st["ks"][li], st["vs"][li]),
                                lora=self._lora_of(li), bias=self._bias_of(li))
            last = x[:, -1]
        else:
            cos, sin, causal = torch_operands()
            for li, w in enumerate(self.layers):
                x = self._layer(x, w, cos, sin, st["kc"][li], st["vc"][li], pidx, causal, lora=self._lora_of(li), bias=self._bias_of(li))
            last = x[:, -1]
        return last

    @torch.no_grad()
    def generate(self, inputs_embeds: Tensor, max_new_tokens: int, use_graph: bool = True, eos_token_id=None, pad_token_id: int = 0,
                 min_new_tokens: int = 0, do_sample: bool = False, temperature: float = 1.0, top_k: Optional[int] = 50, top_p: Optional[float] = 1.0,
                 sample_noise: Optional[Tensor] = None, generator: Optional[torch.Generator] = None, stop_ids=None, text_stop=None,
                 attention_mask: Optional[Tensor] = None, num_beams: int = 1, length_penalty: float = 1.0, repetition_penalty: float = 1.0) -> Tensor:
        """inputs_embeds [B, P, H] -> ids [B, n <= max_new_tokens] (n < max_new_tokens only when every row has finished --
        emitted ``eos_token_id`` or met a stopping keyword -- as HF generate returns them; finished rows are padded).
        ``do_sample``: sample from HF's warped distribution (temperature, top_k [HF's default 50], top_p) with ``sample_noise`` [max_new_tokens, B]
        uniform numbers in [0, 1) (drawn from ``generator`` / the device's default generator when None).  ``stop_ids``: token-id tails that end a
        row when its last ids equal one of them (KeywordsStoppingCriteria's token test, on the device); ``text_stop(ids [1, n]) -> bool``: its
        text test, evaluated on the host for every new length once per 16 tokens (batch 1).  ``attention_mask`` [B, P] of 0 / 1 (None: all ones):
        pads anywhere in the prompt, with HF generate's semantics -- prefill rotary positions ``cumsum(mask) - 1`` (pads at 0), decode step s
        at position ``position_ids[b, P-1] + s`` in cache slot P-1+s, pad keys masked for the whole decode.
        ``num_beams`` > 1: HF's deterministic beam search (``_beam_search``, early_stopping False) with ``length_penalty`` and
        ``repetition_penalty`` -- per batch item the best finished beam, cropped to the longest, finished rows filled with ``pad_token_id or
        eos_token_id``; greedy only, no stopping criteria, the bf16 K/V cache -- or the fp8 one of a decoder built with ``fp8_beams=True`` --
        (NotImplementedError otherwise).
        ``eos_token_id``: None, an id, or a list; a list of several distinct ids is served by a decoder built with ``eos_sets=True`` (up to
        ops.EOS_MAX ids, each in [0, V): any of them ends a row, all are blocked by ``min_new_tokens``, HF's pad default is the first) and
        refused otherwise.
        ``repetition_penalty`` != 1 with one beam: served by a decoder built with ``penalty=True`` -- HF's RepetitionPenaltyLogitsProcessor on
        the fp32 scores of every step over the ids the row has generated (the first token, from the prefill, has none), before the eos block
        of ``min_new_tokens`` and the sampling warpers; greedy or sampled, with every other option -- and refused otherwise."""
        num_beams = int(num_beams)
        if num_beams < 1 or not float(repetition_penalty) > 0.0:
            raise ValueError(f"num_beams={num_beams} / repetition_penalty={repetition_penalty}: at least one beam, a positive penalty")
        if num_beams > 1:
            if do_sample or stop_ids or text_stop is not None:
                raise NotImplementedError("num_beams > 1 with sampling or stopping criteria: use HF generate")
            if self.kv_cache != "bf16" and not self.fp8_beams:
                raise NotImplementedError("num_beams > 1 with kv_cache='fp8': use HF generate")
            return self._generate_beams(inputs_embeds, max_new_tokens, use_graph, eos_token_id, pad_token_id, min_new_tokens, attention_mask, num_beams,
                                        1.0 if length_penalty is None else float(length_penalty), float(repetition_penalty))
        penalty = self._one_beam_penalty(repetition_penalty)
        B, P, _ = inputs_embeds.shape
        pmask = _padding(attention_mask, B, P)
        N = max_new_tokens
        dev, dt = inputs_embeds.device, inputs_embeds.dtype
        eos_token_id, pad_token_id, min_new_tokens = self._special(eos_token_id, pad_token_id, min_new_tokens)
        sample = None
        if do_sample:
            if temperature is None or not float(temperature) > 0.0:
                raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float")      # (HF's TemperatureLogitsWarper)
            sample = (float(temperature), int(top_k) if top_k else 0, float(top_p) if top_p is not None else 1.0)
        stop = tuple(tuple(int(v) for v in t) for t in stop_ids if len(t)) if stop_ids else None
        if text_stop is not None and B != 1:
            raise AssertionError("Only support batch size 1 (yet)")                                          # (the reference's criteria: builder_utils.py:334)
        st = self._state(B, P, N, dev, dt, eos_token_id, pad_token_id, min_new_tokens, sample, stop or None, pmask is not None, penalty)
        if sample is not None:
            if sample_noise is not None:
                st["u"].copy_(sample_noise.to(dev).reshape(N, B))
            else:
                st["u"].copy_(torch.rand(N, B, device=dev, generator=generator))
        ending = eos_token_id is not None or stop is not None or text_stop is not None
        last = self._prefill(st, inputs_embeds, pmask)
        self._reset(st, ending, P)
        first = self._pick(st, self._head(last), 0)      # the first token comes from the prefill, eagerly; the loop replays the other N - 1
        st["tok"].copy_(first)
        st["out"][:, 0] = first
        self._after_token(st, st["step"])
        st["step"].fill_(1)
        return self._replay(st, 1, use_graph, ending, text_stop)


class T5GreedyDecoder(_GraphDecoder):
    """Greedy decode for the seq2seq language model of the BLIP-2 flavours (C1 / C2: Flan-T5 under ``language_model.generate``,
    eval/utils/model.py:432-442; src/models/LSTP_blip2_module.py eval_forward).  HF's generate runs the T5 decoder stack eagerly
    once per token (~1 000 launches per token at 24 layers); here the ENCODER runs once through HF's own module (one pass over
    prefix ‖ prompt -- the seq2seq counterpart of the prefill), the cross-attention K / V of every decoder layer are projected
    once, and ONE decoder step -- embedding, 24 x (self-attention over a static cache with T5's bucketed relative position bias,
    cross-attention, gated-GELU feed-forward), final norm, lm_head, argmax, token / position feedback -- is captured into a
    hipGraph and replayed.  The arithmetic is transformers' modeling_t5 (T5LayerNorm without mean subtraction, unscaled scores,
    bias shared from the first block), so greedy ids equal HF generate's at fp32 (tests/test_decode.py).  Same EOS / pad /
    min_new_tokens semantics and the same return convention as HF for encoder-decoder models: ids start with
    ``decoder_start_token_id``.  Scope: greedy; padded encoder inputs (``attention_mask``) mask the pad keys of the encoder's
    self-attention and of every decoder layer's cross-attention, as HF's extended mask does.  LoRA adapters (train.LoraLinear on q / k / v of
    the encoder's and decoder's SelfAttention and the decoder's EncDecAttention; ``lora_state``) are applied unmerged on every path."""
    _ACT_KIND = {"silu": 0, "swish": 0, "gelu_new": 1, "relu": 2, "gelu": 3}

    def __init__(self, lm, fused: bool = True, weights: str = "bf16", kv_cache: str = "bf16", eos_sets: bool = False, penalty: bool = False):
        cfg = lm.config
        if getattr(cfg, "model_type", "") != "t5":
            raise NotImplementedError("T5GreedyDecoder handles T5ForConditionalGeneration")
        if check_mode("decode_weights", weights) != "bf16":
            raise NotImplementedError(f"decode_weights={weights!r} is implemented for the Llama decoder only")
        if check_mode("kv_cache", kv_cache) != "bf16":
            raise NotImplementedError("kv_cache='fp8' is implemented for the Llama decoder only")
        has_lora = _lora_servable(lm)      # (adapters outside q / k / v of the attention blocks: NotImplementedError)
        super().__init__(lm, fused, weights, kv_cache, eos_sets, penalty)
        self.H, self.dk, self.D = cfg.num_heads, cfg.d_kv, cfg.d_model
        self.eps = cfg.layer_norm_epsilon
        self.start = cfg.decoder_start_token_id if cfg.decoder_start_token_id is not None else cfg.pad_token_id
        self.act_kind = self._ACT_KIND.get(getattr(cfg, "dense_act_fn", None))
        self.layers = []
        for blk in lm.decoder.block:
            sa, ca, ff = blk.layer[0].SelfAttention, blk.layer[1].EncDecAttention, blk.layer[2].DenseReluDense
            wqkv = torch.cat([sa.q.weight, sa.k.weight, sa.v.weight], dim=0).contiguous()
            gated = hasattr(ff, "wi_0")
            wi = torch.cat([ff.wi_0.weight, ff.wi_1.weight], dim=0).contiguous() if gated else ff.wi.weight
            ckv = torch.cat([ca.k.weight, ca.v.weight], dim=0).contiguous()
            self.layers.append(dict(ln0=blk.layer[0].layer_norm.weight, wqkv=wqkv, wo=sa.o.weight, ln1=blk.layer[1].layer_norm.weight,
                                    cq=ca.q.weight, ck=ca.k.weight, cv=ca.v.weight, ckv=ckv, co=ca.o.weight, ln2=blk.layer[2].layer_norm.weight,
                                    wi=wi, wff=ff.wo.weight, act=ff.act, gated=gated))
        # the ENCODER's layers (round 4: prefix || prompt are encoded on libvtgb.so too -- rounds 2-3 called HF's module)
        self.enc_layers = []
        for blk in lm.encoder.block:
            sa, ff = blk.layer[0].SelfAttention, blk.layer[1].DenseReluDense
            gated = hasattr(ff, "wi_0")
            self.enc_layers.append(dict(ln0=blk.layer[0].layer_norm.weight, wqkv=torch.cat([sa.q.weight, sa.k.weight, sa.v.weight], dim=0).contiguous(),
                                        wo=sa.o.weight, ln1=blk.layer[1].layer_norm.weight,
                                        wi=torch.cat([ff.wi_0.weight, ff.wi_1.weight], dim=0).contiguous() if gated else ff.wi.weight,
                                        wff=ff.wo.weight, gated=gated))
        sa0 = lm.decoder.block[0].layer[0].SelfAttention
        self.scaling = float(getattr(sa0, "scaling", 1.0) or 1.0)
        self.bias_module = sa0
        self.enc_bias_module = lm.encoder.block[0].layer[0].SelfAttention
        self.scale_out = bool(getattr(cfg, "scale_decoder_outputs", getattr(cfg, "tie_word_embeddings", False)))
        self._sk: Dict[int, object] = {}          # id(weight) -> its tiled copy for vtgb_gemm_skinny (built on first use)
        # LoRA adapters (train.LoraLinear on q / k / v of the three attention blocks), UNMERGED: per layer the (col0, A, B, scaling) segments of
        # a projection's output, as GreedyDecoder.lora holds them -- references to the model's own fp32 parameters, so a training step is seen
        # without re-packing.  "enc" / "sa": the fused q|k|v of the encoder's / decoder's self-attention; "cq": the cross-attention's q;
        # "ckv": its k | v over the encoder states.  None without adapters: today's launches and allocations.
        self.lora = None
        if has_lora:
            HD = self.H * self.dk

            def segs(att, names):
                return [(i * HD, m.lora_A["default"].weight.detach(), m.lora_B["default"].weight.detach(), float(m.scaling))
                        for i, n in enumerate(names) for m in (getattr(att, n),) if hasattr(m, "lora_A")]
            dec_blocks = lm.decoder.block
            self.lora = dict(enc=[segs(b.layer[0].SelfAttention, _T5_LORA_PROJECTIONS) for b in lm.encoder.block],
                             sa=[segs(b.layer[0].SelfAttention, _T5_LORA_PROJECTIONS) for b in dec_blocks],
                             cq=[segs(b.layer[1].EncDecAttention, ("q",)) for b in dec_blocks],
                             ckv=[segs(b.layer[1].EncDecAttention, ("k", "v")) for b in dec_blocks])

    # ---- libvtgb.so building blocks (round 4: no torch.matmul / F.linear / F.softmax left in the T5 path on the device; the arithmetic is
    # transformers' modeling_t5 with its rounding points: T5LayerNorm = vtgb_llm_rmsnorm, unscaled scores + relative bias, fp32 softmax)
    MAX_KEYS = 2048
    # the decode step's adapted projections (q|k|v, cross q) at bf16: True = the split-K projection with its reduce deferred and ONE
    # vtgb_llm_lora_parts launch that adds the fragments and applies the adapters; False = the materialised projection (projection + reduce
    # launches) and vtgb_llm_lora on top.  The same bits either way (tests/test_gpu_t5_lora.py).  Shipped off: at Flan-T5-XL geometry the one
    # launch is 1.0 % faster per token at B = 1 and 1.8 % slower at B = 8 (profiles/t5_lora_decode_bench.json) -- the update's first phase
    # (A . x), not the launch count, is what the adapters cost.
    LORA_PARTS = False

    def _lora_of(self, which: str, li: int):
        return self.lora[which][li] if self.lora is not None else ()

    def _penalty_start(self) -> Optional[int]:
        # HF's decoder input is the start token: RepetitionPenaltyLogitsProcessor sees it from the first step on
        return int(self.start)

    def _hip(self, x: Tensor) -> bool:
        return (self.fused and x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and self.act_kind is not None
                and (x.dtype == torch.float32 or (self.D % 8 == 0 and (self.H * self.dk) % 8 == 0 and self.cfg.d_ff % 8 == 0)))

    def _lin(self, x: Tensor, w: Tensor, ws: Optional[Tensor] = None) -> Tensor:
        """x [M, K] @ w[N, K]^T on libvtgb.so: the weight-streaming skinny GEMM for a decode step's rows (bf16, M <= 128, K % 64 == 0), else vtgb_gemm."""
        M, K = x.shape
        if x.dtype == torch.bfloat16 and M <= 128 and K % 64 == 0:
            sk = self._sk.get(id(w))
            if sk is None:
                sk = self._sk[id(w)] = ops.SkinnyWeight(w)
            return ops.gemm_skinny(x, sk, workspace=ws)
        return ops.gemm(x, w)

    def _lin_lora(self, x: Tensor, w: Tensor, segs, ws: Optional[Tensor] = None) -> Tensor:
        """``_lin`` with the adapter segments ``segs`` applied to its output (none: ``_lin`` itself)."""
        if not segs:
            return self._lin(x, w, ws)
        M, K = x.shape
        if self.LORA_PARTS and x.dtype == torch.bfloat16 and M <= 128 and K % 64 == 0:
            sk = self._sk.get(id(w))
            if sk is None:
                sk = self._sk[id(w)] = ops.SkinnyWeight(w)
            out, S, part = ops.gemm_skinny(x, sk, workspace=ws, defer_reduce=True)
            if S > 1:      # `out` is not written yet: the fragments are reduced and updated in one launch
                return ops.lora_update_parts(x, out, segs, part, S)
            return ops.lora_update(x, out, segs)
        return ops.lora_update(x, self._lin(x, w, ws), segs)

    @staticmethod
    def _lora_torch(x: Tensor, y: Tensor, segs, shift: int = 0) -> Tensor:
        """The torch statement: y [..., n_cols] with train.LoraLinear.forward's update on the columns of every segment (``shift``: y's first
        column in the segments' numbering; segments before it are another tensor's)."""
        for c0, la, lb, scaling in segs:
            c0, n = c0 - shift, lb.shape[0]
            if 0 <= c0 < y.shape[-1]:
                y = torch.cat((y[..., :c0], y[..., c0: c0 + n] + (F.linear(F.linear(x.to(la.dtype), la), lb) * scaling).to(y.dtype),
                               y[..., c0 + n:]), dim=-1)
        return y

    def _rms(self, x: Tensor, delta: Optional[Tensor], w: Tensor, h: Tensor) -> None:
        L.check(L.lib().vtgb_llm_rmsnorm(dtype_code(x.dtype), _ptr(x), _ptr(delta), _ptr(w), _ptr(h), x.shape[0], x.shape[1], self.eps, _stream()))

    def _attn_rows(self, q: Tensor, q_row: int, k: Tensor, v: Tensor, kv_strides, rows: int, rows_per_batch: int, n_keys: int, t_pad: int,
                   bias: Optional[Tensor], bias_strides, pos: Optional[Tensor], key_valid: Optional[Tensor] = None) -> Tensor:
        out = torch.empty(rows, self.H * self.dk, dtype=q.dtype, device=q.device)
        a = L.LlmAttnRowsArgs(dtype_code(q.dtype), rows, self.H, self.dk, rows_per_batch, n_keys, t_pad, self.scaling, _ptr(q), q_row, _ptr(k), _ptr(v),
                              *kv_strides, _ptr(bias), *bias_strides, _ptr(pos), _ptr(out), self.H * self.dk)
        if key_valid is None:
            L.check(L.lib().vtgb_llm_attention_rows(ctypes.byref(a), _stream()))
        else:      # key_valid [K/V batches, stride] uint8: pad keys of a padded encoder input
            L.check(L.lib().vtgb_llm_attention_rows_masked(ctypes.byref(a), _ptr(key_valid), key_valid.stride(0), _stream()))
        return out

    def _ffn(self, h: Tensor, w: dict, ws: Optional[Tensor] = None) -> Tensor:
        gu = self._lin(h, w["wi"], ws)
        I = gu.shape[1] // 2 if w["gated"] else gu.shape[1]
        act = torch.empty(h.shape[0], I, dtype=h.dtype, device=h.device)
        L.check(L.lib().vtgb_llm_gated_act(dtype_code(h.dtype), _ptr(gu), _ptr(act), h.shape[0], I, self.act_kind, 1 if w["gated"] else 0, _stream()))
        return self._lin(act, w["wff"], ws)

    def _encode_hip(self, inputs_embeds: Tensor, key_valid: Optional[Tensor] = None) -> Tensor:
        """T5Stack (encoder) on libvtgb.so: [B, P, D] -> last_hidden_state [B * P, D] (bias of block 0 shared by every block; ``key_valid``
        [B, P] uint8: a padded input's mask, pad keys get no weight)."""
        B, P, D = inputs_embeds.shape
        HD = self.H * self.dk
        x = inputs_embeds.reshape(B * P, D).clone()
        h = torch.empty_like(x)
        with torch.no_grad():
            bias = self.enc_bias_module.compute_bias(P, P, device=x.device)[0].to(x.dtype).contiguous()      # [H, P (query), P (key)]
        delta = None
        for li, w in enumerate(self.enc_layers):
            self._rms(x, delta, w["ln0"], h)
            qkv = self._lin(h, w["wqkv"])                                                                    # [B P, 3 H dk], token-major
            if self._lora_of("enc", li):
                ops.lora_update(h, qkv, self.lora["enc"][li])
            a = self._attn_rows(qkv, 3 * HD, qkv[:, HD:], qkv[:, 2 * HD:], (P * 3 * HD, self.dk, 3 * HD), B * P, P, P, P, bias, (P, P * P), None,
                                key_valid)
            o = self._lin(a, w["wo"])
            self._rms(x, o, w["ln1"], h)
            delta = self._ffn(h, w)
        enc = torch.empty_like(x)
        self._rms(x, delta, self.lm.encoder.final_layer_norm.weight, enc)
        return enc

    def _decode_step_hip(self, st):
        """One token for every sequence on libvtgb.so (captured): per layer 6 projections (skinny GEMM), T5 norm x 3, cache append,
        self-attention over the static cache with the relative bias row of *pos, cross-attention over the projected encoder states, gated act."""
        lm = self.lm
        B, H, dk, N, Pb = st["tok"].shape[0], self.H, self.dk, st["N"], st["Pb"]
        HD = H * dk
        x, h, q = st["x"], st["h"], st["q"]
        x.copy_(lm.decoder.embed_tokens(st["tok"]))
        ws, pos = st.get("sk_ws"), st["pos"]
        # a beam state (st["attn"] == "beam"): the rows are the B = items x K beams; a row appends its K/V at slot *pos of its own cache row and
        # reads the slots of its ancestry through ``src_row`` (vtgb_llm_attention_rows_beam); the encoder states are the batch item's (K rows each)
        beam = st.get("attn") == "beam"
        K = st["beam"]["K"] if beam else 1
        delta = None
        for li, w in enumerate(self.layers):
            self._rms(x, delta, w["ln0"], h)
            qkv = self._lin_lora(h, w["wqkv"], self._lora_of("sa", li), ws)                                  # [B, 3 H dk] = [B, (q | k | v heads), dk]; adapters before the append
            L.check(L.lib().vtgb_llm_rope_cache(dtype_code(x.dtype), _ptr(qkv), _ptr(q), _ptr(st["kc"][li]), _ptr(st["vc"][li]), None, None, _ptr(pos),
                                                B, H, H, dk, N, _stream()))                                  # (no rotary: cache append)
            if beam:
                a = ops.attention_rows_beam(q, st["kc"][li], st["vc"][li], st["src_row"], pos, self.scaling, bias=st["rel"])
            else:
                a = self._attn_rows(q, HD, st["kc"][li], st["vc"][li], (H * N * dk, N * dk, dk), B, 1, 0, N, st["rel"], (N, N * N), pos)
            o = self._lin(a, w["wo"], ws)
            self._rms(x, o, w["ln1"], h)
            cq = self._lin_lora(h, w["cq"], self._lora_of("cq", li), ws)
            ckv = st["ckv"][li].view(-1, 2 * HD)                                                             # k | v of the encoder states, rows [0, *plen] of every batch entry valid
            a = self._attn_rows(cq, HD, ckv, ckv[:, HD:], (Pb * 2 * HD, dk, 2 * HD), B, K, 0, Pb, None, (0, 0), st["plen"], st.get("ckv_valid"))
            o = self._lin(a, w["co"], ws)
            self._rms(x, o, w["ln2"], h)
            delta = self._ffn(h, w, ws)
        self._rms(x, delta, lm.decoder.final_layer_norm.weight, h)
        hh = h * (self.D ** -0.5) if self.scale_out else h
        (self._beam_emit if beam else self._emit)(st, self._lin(hh, lm.lm_head.weight, ws))

    def _norm(self, x: Tensor, w: Tensor) -> Tensor:
        # T5LayerNorm.forward: fp32 variance, no mean subtraction, no bias; cast to the weight's dtype when it is half / bf16
        var = x.float().pow(2).mean(-1, keepdim=True)
        y = x * torch.rsqrt(var + self.eps)
        if w.dtype in (torch.float16, torch.bfloat16):
            y = y.to(w.dtype)
        return w * y

    def _state(self, B, P, N, device, dtype, eos, pad, min_new, padded=False, beam: Optional[dict] = None, penalty: float = 1.0):
        # On libvtgb.so the encoder length is DEVICE data (`plen`, read by the cross-attention kernel) and the cross-attention K | V live in
        # persistent buffers of a bucketed length (multiples of 64): an eval loop over real questions of varying length reuses a handful of
        # captured graphs (round-3 VERDICT: the state keyed on the exact P).  The torch path (CPU, fused=False) keeps exact-P caches.
        # ``beam`` (K, fill, repetition_penalty, length_penalty; opt-in, beam_search="graph+t5"): a state of R = B * K decoder rows.  On
        # libvtgb.so the encoder's K | V and key mask stay B rows (the cross-attention reads item r / K) and the self-attention caches are
        # kc / vc [R, H, N, dk] -- row r holds what beam row r appended, one slot per decoder position -- read through the int32 ancestry table
        # ``src_row`` [R, N + 1] (slot N is the append target named after the last step and never read); K/V are never copied.  On the torch
        # path the rows keep whole caches, re-ordered by index_select as HF re-orders its cache, and the encoder's K / V are repeated per row.
        hip = self._hip(torch.empty(0, device=device, dtype=dtype))
        if beam is not None and hip and (P > self.MAX_KEYS or N > ops.ATTENTION_ROWS_BEAM_MAX_KEYS):
            raise NotImplementedError(f"num_beams > 1 on the device: up to {self.MAX_KEYS} encoder positions and {ops.ATTENTION_ROWS_BEAM_MAX_KEYS} new "
                                      f"tokens ({P}, {N})")
        hip = hip and P <= self.MAX_KEYS and N <= self.MAX_KEYS
        Pb = -(-P // 64) * 64 if hip else P
        H, dk, nl = self.H, self.dk, len(self.layers)
        items = Be = B                           # batch items; rows of the encoder-side buffers
        if beam is not None:
            B = B * beam["K"]                    # rows of the decoder step
            Be = Be if hip else B

        def z(*shape, dtype=dtype):
            return torch.zeros(*shape, device=device, dtype=dtype)

        def buffers():
            with torch.no_grad():
                bias = self.bias_module.compute_bias(N, N, device=device)[0].permute(1, 0, 2).contiguous().to(dtype)      # [N (query), H, N (key)]
            ar = torch.arange(N, device=device)
            causal = torch.where(ar[None, :] <= ar[:, None], 0.0, torch.finfo(dtype).min).to(dtype)                      # [N, N]
            st = dict(bias=bias + causal[:, None, :], rel=bias.permute(1, 0, 2).contiguous(), N=N, Pb=Pb, hip=hip,      # rel [H, N (query), N (key)]: the kernel's layout (causality = its key range)
                      x=z(B, self.D), h=z(B, self.D), q=z(B, H * dk),
                      # cross-attention K | V of every decoder layer [B, Pb, 2 H dk] (fixed addresses: the captured graph reads them) and the encoder length - 1
                      ckv=[z(Be, Pb, 2 * H * dk) for _ in range(nl)] if hip else [None] * nl, plen=z(1, dtype=torch.long),
                      kc=[z(B, H, N, dk) for _ in range(nl)], vc=[z(B, H, N, dk) for _ in range(nl)],
                      ck=[] if hip else [z(Be, H, P, dk) for _ in range(nl)], cv=[] if hip else [z(Be, H, P, dk) for _ in range(nl)])
            if padded and hip:      # cross-attention key mask over the bucketed encoder length (written before every call)
                st["ckv_valid"] = z(Be, Pb, dtype=torch.uint8)
            elif padded:
                st["cmask"] = z(Be, 1, 1, P)
            if beam is not None:
                K, V = beam["K"], self.lm.lm_head.weight.shape[0]
                st.update(self._beam_book(items, K, N, device, beam["fill"]))
                st.update(beam=dict(beam, kernel=hip), attn="beam" if hip else None, pen_step=z(1, dtype=torch.long),
                          pen_seq=torch.full((B, N + 1), self.start, dtype=torch.long, device=device))
                if hip:
                    st.update(src_row=z(B, N + 1, dtype=torch.int32), row_id=torch.arange(B, dtype=torch.int32, device=device)[:, None],
                              cand_ws=z(ops.beam_candidates_workspace_bytes(B, K, V), dtype=torch.uint8),
                              feedback=("tok", "pos", "step", "src_row") + self.BEAM_BOOK)
            if device.type == "cuda" and dtype == torch.bfloat16 and self.fused and B <= 128:
                shapes = [(3 * H * dk, self.D), (self.D, H * dk), (H * dk, self.D), (self.layers[0]["wi"].shape[0], self.D), (self.D, self.cfg.d_ff),
                          (self.lm.lm_head.weight.shape[0], self.D)]
                need = max([ops.gemm_skinny_workspace_bytes(B, n, k) for n, k in shapes if k % 64 == 0] + [0])
                if need:
                    st["sk_ws"] = z(need, dtype=torch.uint8)
            return st
        key = (B, Pb, N, eos, pad, min_new, hip, padded)
        if beam is not None:      # (keyed by K and the penalties as well: they are constants of the captured step)
            key = ("beams", items, beam["K"], beam["repetition_penalty"], beam["length_penalty"]) + key[1:]
        return self._cached_state(key, B, N, N if beam is None else N + 1, device, eos, pad, min_new, None, None, buffers, penalty)

    def _decode_step(self, st):
        """One token for every sequence, entirely on the device (captured): `tok` at decoder position `pos` -> next token."""
        if st["hip"]:
            return self._decode_step_hip(st)
        lm = self.lm
        B, H, dk = st["tok"].shape[0], self.H, self.dk
        x = lm.decoder.embed_tokens(st["tok"])                                                   # [B, D]
        pos = st["pos"]
        bias = st["bias"].index_select(0, pos)[0][None, :, None, :]                              # [1, H, 1, N]: relative bias + causal mask of this row
        for li, w in enumerate(self.layers):
            h = self._norm(x, w["ln0"])
            qkv = self._lora_torch(h, F.linear(h, w["wqkv"]), self._lora_of("sa", li)).view(B, 3, H, 1, dk)
            st["kc"][li].index_copy_(2, pos, qkv[:, 1])
            st["vc"][li].index_copy_(2, pos, qkv[:, 2])
            sc = torch.matmul(qkv[:, 0], st["kc"][li].transpose(2, 3)) * self.scaling + bias     # [B, H, 1, N]
            a = torch.matmul(F.softmax(sc, dim=-1), st["vc"][li])                                # [B, H, 1, dk]
            x = x + F.linear(a.transpose(1, 2).reshape(B, H * dk), w["wo"])
            h = self._norm(x, w["ln1"])
            q = self._lora_torch(h, F.linear(h, w["cq"]), self._lora_of("cq", li)).view(B, H, 1, dk)
            sc = torch.matmul(q, st["ck"][li].transpose(2, 3)) * self.scaling                    # (no relative bias on cross-attention)
            if "cmask" in st:
                sc = sc + st["cmask"]                                                            # padded encoder input: HF's extended mask
            a = torch.matmul(F.softmax(sc, dim=-1), st["cv"][li])
            x = x + F.linear(a.transpose(1, 2).reshape(B, H * dk), w["co"])
            h = self._norm(x, w["ln2"])
            if w["gated"]:
                gu = F.linear(h, w["wi"])
                half = gu.shape[-1] // 2
                f = w["act"](gu[..., :half]) * gu[..., half:]
            else:
                f = w["act"](F.linear(h, w["wi"]))
            x = x + F.linear(f.to(w["wff"].dtype), w["wff"])
        h = self._norm(x, lm.decoder.final_layer_norm.weight)
        if self.scale_out:
            h = h * (self.D ** -0.5)
        (self._beam_emit if "beam" in st else self._emit)(st, F.linear(h, lm.lm_head.weight))

    # ---- beam search (opt-in at the interfaces: beam_search="graph+t5"): HF's ``_beam_search`` over an encoder-decoder, on the shared bookkeeping of
    # ``_GraphDecoder``.  What differs from the Llama case: every one of the N tokens is a decoder step from the start token (the first runs K
    # identical rows with running scores [0, -1e9, ...]); HF's decoder input is the start token, so ``decoder_prompt_len`` is 1 and the
    # repetition-penalty processor sees that token next to the generated ids -- every length, length-penalty and early-stop count stays the
    # number of generated tokens.
    def _beam_candidates(self, st, logits: Tensor):
        """The shared statement over the ids HF's processors see: the start token, then the ``*step`` generated ids (``pen_seq`` [R, 1 + N] and
        ``pen_step`` = step + 1; the eos block counts generated tokens, so it ends at min_new + 1 of these)."""
        bm, step = st["beam"], st["step"]
        B, K, N = st["run_seq"].shape
        V = logits.shape[-1]
        st["pen_seq"][:, 1:].copy_(st["run_seq"].view(B * K, N))
        st["pen_step"].copy_(step + 1)
        if bm["kernel"] and "eos_t" in st:      # an eos set: the list instantiation of the same kernel
            sc, ix = ops.beam_candidates_eos(logits, st["pen_seq"], st["pen_step"], st["run_scores"], st["eos_t"], bm["repetition_penalty"],
                                             st["min_new"] + 1 if st["min_new"] > 0 else 0, out=(st["cand_score"], st["cand_idx"]),
                                             workspace=st["cand_ws"])
            return sc, ix.long()
        if bm["kernel"]:
            sc, ix = ops.beam_candidates(logits, st["pen_seq"], st["pen_step"], st["run_scores"], bm["repetition_penalty"], st["eos"],
                                         st["min_new"] + 1 if st["min_new"] > 0 else 0, out=(st["cand_score"], st["cand_idx"]), workspace=st["cand_ws"])
            return sc, ix.long()
        lp = F.log_softmax(logits.float(), dim=-1)
        if bm["repetition_penalty"] != 1.0:      # RepetitionPenaltyLogitsProcessor on the log-probabilities; ids behind the step go to a spare column
            ids = torch.where(st["ar"][None, :N + 1] < st["pen_step"], st["pen_seq"], torch.full_like(st["pen_seq"], V))
            lp = torch.cat((lp, torch.zeros_like(lp[:, :1])), dim=-1)
            g = lp.gather(1, ids)
            lp = lp.scatter(1, ids, torch.where(g < 0, g * bm["repetition_penalty"], g / bm["repetition_penalty"]))[:, :V]
        if st["eos"] is not None and st["min_new"] > 0:
            lp = lp.clone()
            for e in (st["eos"] if isinstance(st["eos"], tuple) else (st["eos"],)):      # (an eos set: every id of it)
                lp[:, e] = torch.where(step < st["min_new"], torch.full_like(lp[:, e], float("-inf")), lp[:, e])
        acc = (lp.view(B, K, V) + st["run_scores"][:, :, None]).reshape(B, K * V)
        return torch.topk(acc, k=2 * K)

    def _beam_emit(self, st, logits: Tensor):
        """``_emit`` of a beam state: the selection, then the beams' K/V follow their parents -- the ancestry table on the device
        (src_row' = src_row[parent]; the slot the chosen tokens will be appended at, *step + 1, is the row's own), whole caches elsewhere."""
        rows = self._beam_select(st, logits)
        if st["attn"] == "beam":
            st["src_row"].copy_(st["src_row"].index_select(0, rows))
            st["src_row"].index_copy_(1, st["step"] + 1, st["row_id"])
        else:
            for c in st["kc"] + st["vc"]:
                c.copy_(c.index_select(0, rows))
        st["pos"].add_(1)
        st["step"].add_(1)

    @torch.no_grad()
    def generate(self, inputs_embeds: Tensor, max_new_tokens: int, use_graph: bool = True, eos_token_id=None, pad_token_id: int = 0,
                 min_new_tokens: int = 0, attention_mask: Optional[Tensor] = None, num_beams: int = 1, length_penalty: float = 1.0,
                 repetition_penalty: float = 1.0, do_sample: bool = False, stop_ids=None, text_stop=None) -> Tensor:
        """inputs_embeds [B, P, D] (encoder input) -> ids [B, 1 + n]: decoder_start_token_id, then n <= max_new_tokens
        greedy tokens (n < max_new_tokens only when every row has emitted ``eos_token_id``), as HF generate returns them.
        ``attention_mask`` [B, P] of 0 / 1 (None: all ones): the encoder input's padding.
        ``num_beams`` > 1: HF's deterministic beam search (``_beam_search``, early_stopping False) with ``length_penalty`` and
        ``repetition_penalty`` -- the start token, then per batch item the best finished beam, cropped to the longest, finished rows filled
        with ``pad_token_id or eos_token_id``.  Sampling and stopping criteria are not served (NotImplementedError).  ``repetition_penalty`` != 1
        on one beam: a decoder built with ``penalty=True`` (HF's processor inside the step, over the start token and the generated ids);
        NotImplementedError otherwise.  A list of several distinct eos ids: a decoder built with ``eos_sets=True`` (``GreedyDecoder.generate``)."""
        num_beams = int(num_beams)
        if num_beams < 1 or not float(repetition_penalty) > 0.0:
            raise ValueError(f"num_beams={num_beams} / repetition_penalty={repetition_penalty}: at least one beam, a positive penalty")
        if do_sample or stop_ids or text_stop is not None:
            raise NotImplementedError("T5GreedyDecoder: sampling and stopping criteria are not implemented: use HF generate")
        penalty = self._one_beam_penalty(repetition_penalty) if num_beams == 1 else 1.0      # (beams: the penalty is the beam state's)
        B, P, _ = inputs_embeds.shape
        pmask = _padding(attention_mask, B, P)
        N = max_new_tokens
        dev, dt = inputs_embeds.device, inputs_embeds.dtype
        K, beam = num_beams, None
        rep = (lambda t: t.repeat_interleave(K, 0)) if K > 1 else (lambda t: t)      # (torch path of a beam state: K rows per batch item)
        eos_token_id, pad_token_id, min_new_tokens = self._special(eos_token_id, pad_token_id, min_new_tokens)
        if K > 1:
            if K > ops.BEAM_MAX_BEAMS or 2 * K > self.lm.lm_head.weight.shape[0]:
                raise NotImplementedError(f"num_beams={K}: up to {ops.BEAM_MAX_BEAMS} beams, 2 x num_beams <= vocab_size")
            # HF fills with ``pad_token_id or eos_token_id``: pad 0 fills with eos
            beam = dict(K=K, fill=-1 if eos_token_id is None else int(pad_token_id if pad_token_id else _first_eos(eos_token_id)),
                        repetition_penalty=float(repetition_penalty), length_penalty=1.0 if length_penalty is None else float(length_penalty))
        st = self._state(B, P, N, dev, dt, eos_token_id, beam["fill"] if beam else pad_token_id, min_new_tokens, pmask is not None, beam, penalty)
        valid = None if pmask is None else (pmask.to(dev) != 0)
        if st["hip"]:      # (a beam state too: the encoder and the ckv projections run once per batch item)
            if valid is not None:
                st["ckv_valid"][:, :P].copy_(valid)
            enc = self._encode_hip(inputs_embeds, None if valid is None else valid.to(torch.uint8).contiguous())      # [B P, D]
            st["plen"].fill_(P - 1)
            for li, w in enumerate(self.layers):                                    # cross-attention K | V of every decoder layer, once, into the graph's buffers
                ckv = self._lin(enc, w["ckv"])
                if self._lora_of("ckv", li):      # the adapters of k and v, once per call, before the graph's buffers take the projection
                    ops.lora_update(enc, ckv, self.lora["ckv"][li])
                st["ckv"][li][:, :P].copy_(ckv.view(B, P, 2 * self.H * self.dk))
        else:
            am = torch.ones(B, P, dtype=torch.long, device=dev) if valid is None else valid.long()
            enc = self.lm.encoder(inputs_embeds=inputs_embeds, attention_mask=am).last_hidden_state
            if valid is not None:
                st["cmask"].copy_(rep(torch.where(valid, 0.0, torch.finfo(dt).min).to(dt)[:, None, None, :]))
            for li, w in enumerate(self.layers):
                segs = self._lora_of("ckv", li)
                ck, cv = self._lora_torch(enc, F.linear(enc, w["ck"]), segs), self._lora_torch(enc, F.linear(enc, w["cv"]), segs, self.H * self.dk)
                st["ck"][li].copy_(rep(ck.view(B, P, self.H, self.dk).transpose(1, 2)))
                st["cv"][li].copy_(rep(cv.view(B, P, self.H, self.dk).transpose(1, 2)))
        if beam is not None:
            self._beam_reset(st)
            st["step"].zero_()
            st["pos"].zero_()
            st["tok"].fill_(self.start)
            if st["attn"] == "beam":      # slot 0 holds the start token and is the row's own
                st["src_row"].zero_()
                st["src_row"][:, :1] = st["row_id"]
            self._decode_step(st)         # the first step, eagerly: K identical rows, running scores [0, -1e9, ...]
            out = self._replay_beams(st, use_graph)
            return torch.cat([torch.full((B, 1), self.start, dtype=torch.long, device=dev), out], dim=1)
        self._reset(st, eos_token_id is not None, 0)
        st["tok"].fill_(self.start)                                                 # every one of the N tokens is a replayed step from the start token
        out = self._replay(st, 0, use_graph, eos_token_id is not None)
        return torch.cat([torch.full((B, 1), self.start, dtype=torch.long, device=dev), out], dim=1)


def keyword_stop_plan(criteria) -> dict:
    """``stop_ids`` / ``text_stop`` of GreedyDecoder.generate for a list of KeywordsStoppingCriteria objects (eval/utils/builder_utils.py:320-346; any object
    with ``keyword_ids``, ``keywords``, ``tokenizer``, ``start_len``, ``max_keyword_len``): the id tails of the token test, and the text test as a
    host callback on the generated ids.  (With ``inputs_embeds`` HF's ``output_ids`` holds only generated tokens, so the criteria's
    ``output_ids.shape[1] - start_len`` can be negative; the window arithmetic below is the criteria's own, line 335.)"""
    crit = list(criteria)

    def text_stop(ids):
        for c in crit:
            off = min(ids.shape[1] - c.start_len, c.max_keyword_len)
            text = c.tokenizer.batch_decode(ids[:, -off:], skip_special_tokens=True)[0]
            if any(k in text for k in c.keywords):
                return True
        return False
    return dict(stop_ids=[[int(v) for v in t.tolist()] for c in crit for t in c.keyword_ids], text_stop=text_stop)


def make_decoder(lm, weights: str = "bf16", kv_cache: str = "bf16", fp8_beams: bool = False, eos_sets: bool = False, penalty: bool = False):
    """The graph decoder for a language model: Llama-architecture causal LMs and T5 seq2seq LMs; NotImplementedError otherwise.  The keywords
    are the decoders' own (``DECODER_MODES``); a T5 decoder has no fp8 cache and does not take ``fp8_beams``."""
    if getattr(lm.config, "model_type", "") == "t5":
        return T5GreedyDecoder(lm, weights=weights, kv_cache=kv_cache, eos_sets=eos_sets, penalty=penalty)
    return GreedyDecoder(lm, weights=weights, kv_cache=kv_cache, fp8_beams=fp8_beams, eos_sets=eos_sets, penalty=penalty)


def prompt_padding(attention_mask: Tensor) -> Tuple[Optional[bool], Tensor]:
    """(padded, host copy) of a prompt mask [B, P], with ONE device-to-host copy: padded is False for all ones, True for a padded mask,
    None outside the decoders' envelope (values other than 0 / 1, or a row without a token -- HF generate runs those).  Callers hand
    the host copy on to the decoders, whose own check of a host tensor reads no device memory."""
    m = attention_mask.detach().cpu()
    if not bool(((m == 0) | (m == 1)).all()) or not bool((m != 0).any(-1).all()):
        return None, m
    return not bool((m != 0).all()), m


def decoder_for(owner, lm):
    """The graph decoder for ``lm``, cached on ``owner`` (attribute ``_decoder``): the cached one when it was built for this ``lm`` and the
    weights it re-packed are still the model's (``weights_key``) and its ``DECODER_MODES`` attributes are those of the owner's modes (``modes_of``,
    read on every call), else a new one: ``make_decoder`` with the modes that are not the default -- by default the positional ``lm`` alone."""
    want, default = modes_of(owner)._asdict(), DecodeModes._field_defaults
    dec = getattr(owner, "_decoder", None)
    # (an attribute a decoder lacks counts as the default; a T5 decoder has no ``fp8_beams`` and is not retired for it)
    if dec is None or dec.lm is not lm or dec.key != weights_key(lm) or any(
            getattr(dec, f, want[f] if f == "fp8_beams" else default[f]) != want[f] for f in DECODER_MODES):
        dec = owner._decoder = make_decoder(lm, **{f: want[f] for f in DECODER_MODES if want[f] != default[f]})
    return dec


class Envelope(NamedTuple):
    """What a caller lets the graph decoders serve: the request keys it knows, the values of beam / penalty keys that leave the ids those of
    plain decoding, whether sampling is served (Llama), whether ``max_new_tokens`` must be in the request."""
    keys: frozenset
    neutral: dict
    sampling: bool
    # the request must give its length: as ``max_new_tokens``, or -- in an envelope whose ``keys`` hold "max_length" (the beam and sampled
    # twins of the module envelope) -- as HF's ``max_length``, which ``graph_generate`` resolves with ``generated_length``
    need_max_new: bool
    # opt-in (eos_sets="graph"): several distinct eos ids (up to ops.EOS_MAX, each in [0, vocab_size)) stay on the decoders.  Always given by
    # name (``_replace(eos_sets=True)``); it stands before the beam switches because tests/test_t5_beam_decode.py pins those as the last two fields
    eos_sets: bool = False
    # opt-in (penalty_decode="graph"): a one-beam request may carry any real ``repetition_penalty`` > 0 (Llama and T5; greedy, and sampling where
    # ``sampling`` serves it).  Always given by name, and placed before the beam switches for the same reason
    penalty: bool = False
    beams: bool = False      # opt-in (beam_search="graph"): Llama, num_beams > 1 with any positive repetition_penalty and any length_penalty
    t5_beams: bool = False   # opt-in (beam_search="graph+t5"): the same requests on a T5 as well


_COMMON_KEYS = {"do_sample", "temperature", "top_p", "min_new_tokens", "eos_token_id", "pad_token_id", "num_beams", "repetition_penalty", "length_penalty"}
_LENGTH_KEYS = {"max_length", "min_length"}      # HF's way to give the length (``generated_length``), as the shipped generate_configs do
_BASE_ENVELOPES = {
    # LSTP.generate(**gen_kwargs): sampling and KeywordsStoppingCriteria on Llama (max_new_tokens / use_cache are its own parameters, handed to the
    # decoder by the caller)
    False: Envelope(frozenset(_COMMON_KEYS | {"top_k", "sample_noise", "generator", "stopping_criteria"}),
                    {"num_beams": (1,), "repetition_penalty": (None, 1.0), "length_penalty": (None, 1.0)}, sampling=True, need_max_new=False),
    # the LightningModule twins' ``generate_configs``: greedy only (length_penalty has no effect on one beam)
    True: Envelope(frozenset(_COMMON_KEYS | {"max_new_tokens", "use_cache"}), {"num_beams": (1,), "repetition_penalty": (1.0,)},
                   sampling=False, need_max_new=True)}


@functools.lru_cache(maxsize=None)      # (one object per envelope: callers and tests compare them with ``is``)
def _envelope(module: bool, beams: bool, t5_beams: bool, eos_sets: bool, sampled: bool, penalty: bool) -> Envelope:
    """The envelope of LSTP.generate (``module`` False) or of the LightningModule twins under the envelope half of a ``DecodeModes``."""
    env = _BASE_ENVELOPES[module]
    if beams:      # deterministic beam search on Llama; the modules' configurations may then give the length as ``max_length`` / ``min_length``
        env = env._replace(keys=env.keys | _LENGTH_KEYS if module else env.keys, beams=True)
    if t5_beams:      # a T5's beam requests as well
        env = env._replace(t5_beams=True)
    if eos_sets:
        env = env._replace(eos_sets=True)
    if module and sampled:      # the modules' configurations may sample and give the length that way (LSTP.generate's envelope samples already)
        env = env._replace(sampling=True, keys=env.keys | _LENGTH_KEYS)
    if penalty:
        env = env._replace(penalty=True)
    return env


GENERATE_ENVELOPE, MODULE_ENVELOPE = (_envelope(m, False, False, False, False, False) for m in (False, True))
GENERATE_ENVELOPE_BEAMS, MODULE_ENVELOPE_BEAMS = (_envelope(m, True, False, False, False, False) for m in (False, True))               # beam_search="graph"
GENERATE_ENVELOPE_T5_BEAMS, MODULE_ENVELOPE_T5_BEAMS = (_envelope(m, True, True, False, False, False) for m in (False, True))          # "graph+t5"


def envelope_for(owner, module: bool) -> Envelope:
    """The envelope a caller plans with: ``_envelope`` of the owner's modes (``modes_of``, read on every call).  With no opt-in but
    ``beam_search`` it is one of the six objects above; ``sampled_decode`` changes the module envelope alone, "+kv8" the decoder alone."""
    m, module = modes_of(owner), bool(module)
    return _envelope(module, m.beams, m.t5_beams, m.eos_sets, module and m.sampled, m.penalty)


def generated_length(lm, request: dict, P: int) -> Optional[Tuple[int, Optional[int]]]:
    """(max_new_tokens, min_new_tokens from ``min_length`` or None) of a request with HF's ``_prepare_generated_length`` semantics:
    ``max_new_tokens`` wins over ``max_length``; a Llama over embeddings generates ``max_length - P`` tokens and blocks eos for
    ``max(min_length - P, 0)``; T5 starts from one decoder token: ``max_length - 1`` and ``max(min_length - 1, 0)``.  None: no length given."""
    used = 1 if getattr(lm.config, "model_type", "") == "t5" else P
    if request.get("max_new_tokens") is not None:
        n = int(request["max_new_tokens"])
    elif request.get("max_length") is not None:
        n = int(request["max_length"]) - used
    else:
        return None
    return n, (max(int(request["min_length"]) - used, 0) if request.get("min_length") is not None else None)


def plan_decode(lm, inputs_embeds, attention_mask: Tensor, request: dict, env: Envelope) -> Optional[dict]:
    """The keyword arguments of ``decoder_for(owner, lm).generate(inputs_embeds, max_new_tokens, **plan)`` for a request HF ``generate`` would get
    as ``generate(inputs_embeds=..., attention_mask=..., **request)``, or None when it is outside what the graph decoders reproduce (then HF
    ``generate`` runs it).  Inside: a Llama the decoder states (``llama_state``) or a T5 language model on the device, at most one distinct eos
    id (under ``env.eos_sets``: up to ops.EOS_MAX, each in [0, vocab_size)), only keys ``env`` knows, one beam, neutral penalties (or, where
    ``env.beams`` -- for a T5 ``env.t5_beams`` -- says so, deterministic beam search with a positive repetition penalty; under ``env.penalty``
    one beam with any finite positive repetition penalty, which enters the plan when it is not 1), a 0 / 1
    attention mask with a token in every row (a padded mask goes into the plan as its host copy); greedy, or -- Llama, where ``env`` serves it --
    sampling with temperature / top_k / top_p; ``stopping_criteria`` None or (Llama) KeywordsStoppingCriteria objects (eval/utils/builder_utils.py:
    320-346: recognised by their ``keyword_ids`` / ``keywords`` / ``tokenizer`` attributes)."""
    def number(v, types=(int, float)):      # (a bool is an int to Python and no number to HF generate)
        return isinstance(v, types) and not isinstance(v, bool)
    mt = getattr(lm.config, "model_type", "")
    if not inputs_embeds.is_cuda or not ("llama" in mt or mt == "t5"):
        return None
    if set(request) - env.keys or (env.need_max_new and "max_new_tokens" not in request and not ("max_length" in env.keys and request.get("max_length") is not None)):
        return None
    if lora_state(lm) not in (None, "ok"):      # adapters the decoders do not apply: HF generate runs the modules' own forward
        return None
    if "llama" in mt and llama_state(lm) is not None:      # a Llama the decoder does not state (rope type, lm_head bias, ...): HF generate
        return None
    do_sample = bool(request.get("do_sample", False))
    crit = list(request["stopping_criteria"]) if request.get("stopping_criteria") is not None else []
    K = request.get("num_beams", 1)
    beams = env.beams and number(K, int) and K > 1
    if beams:      # deterministic beam search on Llama (on T5: under ``env.t5_beams``); any positive repetition penalty, any length penalty
        rp, lp = request.get("repetition_penalty"), request.get("length_penalty")
        rp, lp = (1.0 if rp is None else rp), (1.0 if lp is None else lp)
        if not ("llama" in mt or (mt == "t5" and env.t5_beams)) or do_sample or crit or not (number(rp) and number(lp)) or not rp > 0:
            return None
    elif any(k in request and request[k] not in ok for k, ok in env.neutral.items() if not (env.penalty and k == "repetition_penalty")):
        return None
    one_pen = 1.0      # one beam under ``env.penalty``: any real repetition penalty > 0 (None counts as 1); anything else is HF generate's to judge
    if env.penalty and not beams:
        one_pen = request.get("repetition_penalty")
        one_pen = 1.0 if one_pen is None else one_pen
        if not number(one_pen) or not 0 < one_pen < float("inf"):
            return None
    if (do_sample and not env.sampling) or any(not all(hasattr(c, a) for a in ("keyword_ids", "keywords", "tokenizer")) for c in crit):
        return None
    if mt == "t5" and (do_sample or crit):
        return None
    padded, host_mask = prompt_padding(attention_mask)
    if padded is None:
        return None
    gc = getattr(lm, "generation_config", None)     # HF generate's defaults come from the generation config
    eos = request.get("eos_token_id", getattr(gc, "eos_token_id", None))
    if isinstance(eos, (list, tuple)) and len(set(eos)) > 1:      # several distinct eos ids (Llama-3.1-Instruct ships three): HF generate,
        # or -- under ``env.eos_sets`` -- the decoders' eos sets: up to ops.EOS_MAX ids, each a token of the vocabulary
        V = getattr(lm.config, "vocab_size", 0)
        if not env.eos_sets or len(set(eos)) > ops.EOS_MAX or any(not number(e, int) or not 0 <= e < V for e in eos):
            return None
        eos = list(eos)
    elif isinstance(eos, (list, tuple)) and len(eos) > 1:      # (one id, repeated)
        eos = [eos[0]]
    plan = dict(eos_token_id=eos,
                pad_token_id=request.get("pad_token_id", getattr(gc, "pad_token_id", None)), min_new_tokens=int(request.get("min_new_tokens", 0) or 0))
    if padded:
        plan["attention_mask"] = host_mask      # (the host copy: the decoder classifies it again without reading the device)
    if do_sample:
        plan.update(do_sample=True, temperature=request.get("temperature"), top_k=request.get("top_k", getattr(gc, "top_k", 50)),
                    top_p=request.get("top_p", getattr(gc, "top_p", 1.0)), sample_noise=request.get("sample_noise"), generator=request.get("generator"))
    if crit:
        if inputs_embeds.shape[0] != 1:
            raise AssertionError("Only support batch size 1 (yet)")      # (the reference's criteria)
        plan.update(keyword_stop_plan(crit))
    if beams:
        plan.update(num_beams=K, repetition_penalty=float(rp), length_penalty=float(lp))
    elif one_pen != 1:      # (a neutral penalty plans exactly as without the opt-in)
        plan["repetition_penalty"] = float(one_pen)
    return plan


def graph_generate(owner, lm, inputs_embeds: Tensor, attention_mask: Tensor, generate_configs: dict):
    """``lm.generate(inputs_embeds=..., attention_mask=..., **generate_configs)`` through the graph decoder when the configuration is inside
    the owner's module envelope (``envelope_for``: MODULE_ENVELOPE, or what the owner's ``MODES`` make of it), else None (the caller then runs
    HF generate).  The decoder is cached on ``owner`` (``decoder_for``)."""
    gc = dict(generate_configs or {})
    env = envelope_for(owner, module=True)
    plan = plan_decode(lm, inputs_embeds, attention_mask, gc, env)
    if plan is None:
        return None
    if "max_length" not in env.keys:      # (the length is ``max_new_tokens``: ``need_max_new``)
        return decoder_for(owner, lm).generate(inputs_embeds, int(gc["max_new_tokens"]), **plan)
    n, min_new = generated_length(lm, gc, inputs_embeds.shape[1])
    if n <= 0:      # HF generate reports it in its own words
        return None
    if gc.get("min_new_tokens") is None and min_new is not None:      # (min_new_tokens wins over min_length, as in HF)
        plan["min_new_tokens"] = min_new
    return decoder_for(owner, lm).generate(inputs_embeds, n, **plan)
