"""Clip sessions: many questions about one clip, the question-independent work done once.

``LSTP.generate`` repeats the whole path for every question: RAFT over the clip's frame pairs, the TGB, ViT-g over the selected
frames, the Q-Former and the decode.  Much of that does not depend on the question (the QA benchmarks ask 10-25 questions per
video; the reference's demo keeps a video's state across turns the same way, demo/demo.py:42-72):

  RAFT flow            -- the frames alone: once per session;
  TGB trunk            -- TemporalOFEmbedding + LayerNorm and the layers before the first cross-attention layer (multi_modal:
                          [0, fusion_layer); fusion: none): once per session (vtgb_tgb_trunk), resumed per question (vtgb_tgb_resume);
  ViT-g per frame      -- a frame's embedding does not depend on the question: each candidate frame is encoded at most once, on the
                          first question that selects it, into a bank [N, tokens, hidden] in the compute dtype;
  BLIP-2 Q-Former      -- no text branch, so its output per frame is banked too ([N, n_query, hidden]).

Every stage's result for a row does not depend on the batch it runs in ("determinism and batch invariance"), and the session
runs RAFT on one clip exactly as a one-clip ``generate`` does, so ``sess.generate`` returns what ``model.generate`` returns for the same
question, BIT FOR BIT (tests/test_gpu_session.py)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops

Tensor = torch.Tensor


def _param_key(module) -> tuple:
    return tuple((p._version, p.data_ptr()) for p in module.parameters()) + tuple((b._version, b.data_ptr()) for b in module.buffers())


class ClipSession:
    """Built by ``model.clip_session(frames, flow_frames)`` / ``model.clip_session(frames, of=of)``; see ``generate``."""

    def __init__(self, model, frames: Tensor, flow_frames: Optional[Tensor] = None, of: Optional[Tensor] = None):
        if frames.dim() == 5:
            if frames.shape[0] != 1:
                raise ValueError(f"clip_session: frames {tuple(frames.shape)} hold {frames.shape[0]} clips; a session is one clip")
            frames = frames[0]
        if frames.dim() != 4:
            raise ValueError(f"clip_session: frames {tuple(frames.shape)} are not one clip's candidates [N, 3, S, S]")
        if of is None:
            if flow_frames is None:
                raise ValueError("clip_session: give flow_frames [1, T, 3, S, S] or a precomputed flow of [1, T, 2, S, S]")
            if flow_frames.dim() != 5 or flow_frames.shape[0] != 1:
                raise ValueError(f"clip_session: flow_frames {tuple(flow_frames.shape)} are not one clip [1, T, 3, S, S]")
        elif of.dim() != 5 or of.shape[0] != 1:
            raise ValueError(f"clip_session: of {tuple(of.shape)} is not one clip's flow [1, T, 2, S, S]")
        self.model = model
        self.frames = frames.contiguous().float()          # (what generate's gather reads: pixel_values.contiguous().float())
        self.N = self.frames.shape[0]
        self.raft_calls = 0
        self._own_flow = of is None
        if of is None:
            of = model.flow(flow_frames)
            self.raft_calls = 1
        self.of = of
        self.T = of.shape[1]
        self.of_mask = torch.ones(1, self.T + 2, dtype=torch.long, device=of.device)
        self.trunk = model.temporal_encoder.trunk(encoder_embeds=of, attention_mask=self.of_mask, mode=model.TGB_MODE)
        self.bank: Optional[Tensor] = None                 # ViT last_hidden_state per candidate frame, compute dtype
        self.qbank: Optional[Tensor] = None                # BLIP-2: Q-Former query rows per candidate frame, fp32
        self.filled = np.zeros(self.N, dtype=bool)
        self.vit_frames_encoded = 0
        self._key = self._weights_key()

    # ---- staleness -------------------------------------------------------------------------------------------------------------
    def _weights_key(self) -> tuple:
        """(in-place version, storage address) of every tensor the cached state was computed from, and the stages' compute dtypes: a
        load_state_dict, an optimizer step, a ``.to()`` or set_compute_dtype on the model changes it (the idea of decode.weights_key and
        models._Stage._versions).  The language model and the projection are not cached here: each call reads them afresh."""
        m = self.model
        pm = m.model
        key = (m.temporal_encoder.code, pm.vision_model.code, pm.qformer.code, m.temporal_encoder._versions(), pm.vision_model._versions(),
               pm.qformer._versions(), (pm.query_tokens._version, pm.query_tokens.data_ptr()))
        if self._own_flow:
            key += (m.of_extractor.code, _param_key(m.of_extractor))
        return key

    def _check_fresh(self) -> None:
        if self._weights_key() != self._key:
            raise RuntimeError("clip session is stale: the model's weights or compute dtype changed after the session was built "
                               "(load_state_dict / optimizer step / set_compute_dtype / .to()); build a new session with model.clip_session(...)")

    # ---- the frame bank --------------------------------------------------------------------------------------------------------
    def _encode(self, ids) -> None:
        """ViT (and, for BLIP-2, the Q-Former) over the candidate frames ``ids`` not encoded yet, in one call each."""
        new = [int(i) for i in ids if not self.filled[int(i)]]
        if not new:
            return
        m = self.model
        sel = torch.tensor(new, dtype=torch.long, device=self.frames.device)
        img = m.model.vision_model(pixel_values=self.frames.index_select(0, sel), return_dict=True, act_output=True).last_hidden_state
        if self.bank is None:
            self.bank = torch.empty((self.N,) + tuple(img.shape[1:]), dtype=img.dtype, device=img.device)
        self.bank[sel] = img
        if m.ARCH != "instructblip":
            qo = m._query_rows(img, 1)
            if self.qbank is None:
                self.qbank = torch.empty((self.N,) + tuple(qo.shape[1:]), dtype=qo.dtype, device=qo.device)
            self.qbank[sel] = qo
        self.filled[new] = True
        self.vit_frames_encoded += len(new)

    @torch.no_grad()
    def prefetch(self) -> "ClipSession":
        """Encode all N candidate frames at once (for callers who know many questions will follow)."""
        self._check_fresh()
        self._encode(range(self.N))
        return self

    # ---- questions -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, nframe, text_encoding, sampler_text_encoding, do_sample=True, temperature=0.2, max_new_tokens=1024, use_cache=True,
                 stopping_criteria=None, noise: Optional[Tensor] = None, pool: str = "mean", return_stages: bool = False, fast_decode="auto",
                 **gen_kwargs):
        """``model.generate``'s question-side arguments, same meaning; B = rows of ``sampler_text_encoding``, every row a question about the
        session's clip; ``noise`` [2, 2B, T] as generate takes it for B rows.  Returns what ``model.generate(frames, flow_frames, ...)`` returns
        for these questions: (ids, cand_index[, stages]).  Questions of different lengths go in one call padded (``attention_mask`` 0 on the
        pads, e.g. the tokenizer's padding="longest"): the graph decoder takes the padded batch with HF generate's padding semantics."""
        self._check_fresh()
        m = self.model
        sampler_ids = sampler_text_encoding["input_ids"]
        B = sampler_ids.shape[0]
        if text_encoding["input_ids"].shape[0] != B:
            raise ValueError(f"clip session: text_encoding has {text_encoding['input_ids'].shape[0]} rows, sampler_text_encoding {B}")
        if m.ARCH == "instructblip" and text_encoding["qformer_input_ids"].shape[0] != B:
            raise ValueError(f"clip session: qformer_input_ids has {text_encoding['qformer_input_ids'].shape[0]} rows, sampler_text_encoding {B}")
        if nframe > self.N:
            raise ValueError(f"clip session: nframe {nframe} exceeds the clip's {self.N} candidate frames")
        # TGB resumed from the trunk -> Gumbel top-k -> index map (select_frames' arithmetic)
        _, logits = m.temporal_encoder.resume(self.trunk, encoder_hidden_states=sampler_ids,
                                              encoder_attention_mask=sampler_text_encoding["attention_mask"])
        if noise is None:   # F.gumbel_softmax's noise: -log(Exp(1)), fresh per draw (Appendix B)
            noise = -torch.empty(2, 2 * B, self.T, device=self.of.device).exponential_().log()
        sel = ops.span_select(logits, noise, 0.5)
        idx = ops.span_to_frames(sel, self.T, self.N, nframe, m.MAP)
        self._encode(np.unique(idx.cpu().numpy()))         # the one host read of a call
        flat = idx.reshape(-1)
        if m.ARCH == "instructblip":
            qo = m._query_rows(self.bank.index_select(0, flat), nframe, text_encoding)
        else:
            qo = self.qbank.index_select(0, flat)
        lm_inputs = m._pool_project(qo, B, nframe, pool)
        outputs, lm_inputs, inputs_embeds = m._decode(lm_inputs, text_encoding, do_sample, temperature, max_new_tokens, use_cache,
                                                      stopping_criteria, fast_decode, gen_kwargs)
        cand_index = idx[-1]
        if return_stages:
            of = self.of if B == 1 else self.of.expand(B, *self.of.shape[1:])
            sampled = self.frames.index_select(0, flat)
            return outputs, cand_index, dict(of=of, tgb_logits=logits, frame_idx=idx, sampled=sampled, prefix=lm_inputs,
                                             inputs_embeds=inputs_embeds)
        return outputs, cand_index
