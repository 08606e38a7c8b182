"""The float64 statements of tests/train_llm_ref.py against HF's own modules and torch autograd, on the CPU: what
tests/test_gpu_train_llm.py holds the kernels of csrc/train_llm.hip and ``train.llama_with_grad`` to is what transformers computes."""
import math

import pytest
import torch

import train_llm_ref as R

TOL = 1e-12      # float64 on both sides: rounding of a different operation order only
HF32 = 2e-6      # LlamaRMSNorm normalises, and eager_attention_forward takes its softmax, in float32 whatever the module's dtype: a few fp32 ulps


def _close(a, b, tol=TOL):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def _config(**kw):
    from transformers import LlamaConfig
    d = dict(hidden_size=32, intermediate_size=48, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=50,
             attn_implementation="eager")
    d.update(kw)
    return LlamaConfig(**d)


@pytest.mark.parametrize("use_delta", [False, True])
def test_rmsnorm_statement_is_llama_rmsnorm_with_the_residual_add(use_delta):
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    g = torch.Generator().manual_seed(1)
    D, eps = 32, 1e-6
    norm = LlamaRMSNorm(D, eps=eps).double()
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(D, generator=g))
    x = torch.randn(3, 5, D, generator=g, dtype=torch.float64).requires_grad_(True)
    delta = torch.randn(3, 5, D, generator=g, dtype=torch.float64).requires_grad_(True) if use_delta else None
    w = torch.randn(3, 5, D, generator=g, dtype=torch.float64)
    w2 = torch.randn(3, 5, D, generator=g, dtype=torch.float64)          # what the residual stream's later consumers return
    resid = x + delta if use_delta else x
    want = norm(resid)
    ((want * w).sum() + (resid * w2).sum()).backward()
    y, s, rstd = R.rmsnorm_forward(x.detach(), None if delta is None else delta.detach(), norm.weight.detach(), eps)
    assert _close(y, want.detach(), HF32) and _close(s, resid.detach())
    ds = R.rmsnorm_backward(w, s, rstd, norm.weight.detach(), dsum=w2)
    assert _close(ds, x.grad, HF32)
    if use_delta:
        assert _close(ds, delta.grad, HF32)
    # the backward formula against autograd of the forward statement, float64 throughout
    x2 = x.detach().clone().requires_grad_(True)
    y2, s2, _ = R.rmsnorm_forward(x2, None if delta is None else delta.detach(), norm.weight.detach(), eps)
    ((y2 * w).sum() + (s2 * w2).sum()).backward()
    assert _close(ds, x2.grad)


@pytest.mark.parametrize("nh,nkv,hd", [(2, 2, 16), (8, 2, 64)])
def test_rope_statement_is_apply_rotary_pos_emb_and_conjugate_is_its_vjp(nh, nkv, hd):
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding, apply_rotary_pos_emb
    g = torch.Generator().manual_seed(2)
    B, S = 2, 5
    cfg = _config(hidden_size=nh * hd, num_attention_heads=nh, num_key_value_heads=nkv)
    rot = LlamaRotaryEmbedding(cfg)
    x = torch.randn(B, S, (nh + 2 * nkv) * hd, generator=g, dtype=torch.float64)
    cos, sin = rot(x, torch.arange(S)[None])                             # [1, S, hd]
    q, k, v = x.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    qh, kh = q.view(B, S, nh, hd).transpose(1, 2), k.view(B, S, nkv, hd).transpose(1, 2)
    qr, kr = apply_rotary_pos_emb(qh, kh, cos, sin)
    want = torch.cat([qr.transpose(1, 2).reshape(B, S, -1), kr.transpose(1, 2).reshape(B, S, -1), v], dim=-1)
    got = R.rope(x, cos[0].double(), sin[0].double(), nh, nkv, hd)
    assert _close(got, want)
    # the conjugate launch is the vector-Jacobian product -- for ANY table, not only one whose two halves agree
    for c, s in ((cos[0].double(), sin[0].double()), (torch.randn(S, hd, generator=g, dtype=torch.float64), torch.randn(S, hd, generator=g, dtype=torch.float64))):
        xx = x.clone().requires_grad_(True)
        w = torch.randn(x.shape, generator=g, dtype=torch.float64)
        (R.rope(xx, c, s, nh, nkv, hd) * w).sum().backward()
        assert _close(R.rope(w, c, s, nh, nkv, hd, conjugate=True), xx.grad)
    # and, for a rotation (HF's table: cos^2 + sin^2 = 1 to the rounding of its fp32 entries), its inverse
    assert _close(R.rope(got, cos[0].double(), sin[0].double(), nh, nkv, hd, conjugate=True), x, HF32)


def test_swiglu_statement_is_llama_mlp():
    from transformers.models.llama.modeling_llama import LlamaMLP
    g = torch.Generator().manual_seed(3)
    mlp = LlamaMLP(_config()).double()
    x = torch.randn(2, 7, 32, generator=g, dtype=torch.float64)
    gu = torch.cat([mlp.gate_proj(x), mlp.up_proj(x)], dim=-1).detach().requires_grad_(True)
    assert _close(mlp.down_proj(R.swiglu_forward(gu)), mlp(x))
    w = torch.randn(2, 7, 48, generator=g, dtype=torch.float64)
    I = 48
    (torch.nn.functional.silu(gu[..., :I]) * gu[..., I:] * w).sum().backward()
    assert _close(R.swiglu_backward(gu.detach(), w), gu.grad)


def _hf_mask(attention_mask, S, dtype):
    """The additive 4-D mask HF builds from a 0 / 1 padding mask: causal AND not padded, dtype.min elsewhere."""
    keep = torch.ones(S, S, dtype=torch.bool).tril()[None, None] & (attention_mask[:, None, None, :] != 0)
    return torch.zeros(attention_mask.shape[0], 1, S, S, dtype=dtype).masked_fill(~keep, torch.finfo(dtype).min)


@pytest.mark.parametrize("nh,nkv", [(4, 2), (4, 4), (4, 1)])
def test_attention_statement_is_eager_llama_attention_causal_padded_grouped(nh, nkv):
    from transformers.models.llama.modeling_llama import LlamaAttention, LlamaRotaryEmbedding
    g = torch.Generator().manual_seed(4)
    cfg = _config(num_attention_heads=nh, num_key_value_heads=nkv)
    hd, B, S = 32 // nh, 2, 9
    att = LlamaAttention(cfg, layer_idx=0).double().eval()
    hidden = torch.randn(B, S, 32, generator=g, dtype=torch.float64).requires_grad_(True)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 6:] = 0                                                            # right padding: every row keeps a visible key
    cos, sin = LlamaRotaryEmbedding(cfg)(hidden, torch.arange(S)[None])
    cos, sin = cos.double(), sin.double()
    want, _ = att(hidden, position_embeddings=(cos, sin), attention_mask=_hf_mask(am, S, torch.float64))
    w = torch.randn(B, S, 32, generator=g, dtype=torch.float64) * am[..., None]      # (padded query rows carry no loss)
    (want * w).sum().backward()
    # the statement: projections -> rope -> causal grouped attention with the additive key mask -> o_proj
    key_mask = torch.zeros(B, S, dtype=torch.float64).masked_fill(am == 0, torch.finfo(torch.float32).min)
    h2 = hidden.detach().clone().requires_grad_(True)
    qkv = R.rope(torch.cat([att.q_proj(h2), att.k_proj(h2), att.v_proj(h2)], dim=-1), cos[0], sin[0], nh, nkv, hd)
    q, k, v = (t.detach().requires_grad_(True) for t in qkv.split([nh * hd, nkv * hd, nkv * hd], dim=-1))
    out, lse = R.attn_causal_forward(q, k, v, nh, nkv, 1.0 / math.sqrt(hd), key_mask)
    got = att.o_proj(out)
    valid = am[..., None].double()
    assert _close(got * valid, want.detach() * valid, HF32)
    # the backward formulas against autograd of the forward statement ...
    go = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * go).sum().backward()
    dq, dk, dv = R.attn_causal_backward(q.detach(), k.detach(), v.detach(), out.detach(), lse.detach(), go, nh, nkv, 1.0 / math.sqrt(hd), key_mask)
    assert _close(dq, q.grad) and _close(dk, k.grad) and _close(dv, v.grad)
    # ... and the gradient of the whole block against HF's
    qkv2 = R.rope(torch.cat([att.q_proj(h2), att.k_proj(h2), att.v_proj(h2)], dim=-1), cos[0], sin[0], nh, nkv, hd)
    q2, k2, v2 = qkv2.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    (att.o_proj(R.attn_causal_forward(q2, k2, v2, nh, nkv, 1.0 / math.sqrt(hd), key_mask)[0]) * w).sum().backward()
    assert _close(h2.grad, hidden.grad, HF32)


def test_a_query_row_without_a_visible_key_stays_finite():
    g = torch.Generator().manual_seed(5)
    B, S, nh, hd = 1, 6, 2, 8
    q, k, v = (torch.randn(B, S, nh * hd, generator=g, dtype=torch.float64) for _ in range(3))
    key_mask = torch.zeros(B, S, dtype=torch.float64)
    key_mask[0, :3] = torch.finfo(torch.float32).min                         # left padding: rows 0 .. 2 see masked keys only
    out, lse = R.attn_causal_forward(q, k, v, nh, nh, hd ** -0.5, key_mask)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()


@pytest.mark.parametrize("kv_heads,targets", [(2, None), (1, ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"))])
def test_model_statement_is_hf_llama_with_lora(kv_heads, targets):
    """llama_logits (layers of llama_layer, final norm, lm_head) against LlamaForCausalLM.forward in float64, adapters on; loss gradients of the
    adapters and of the inputs against HF + autograd."""
    from videotgb_amd import llm, train
    lm = llm.build_llama("tiny", torch.float64, "cpu", num_key_value_heads=kv_heads, attn_implementation="eager")
    train.apply_lora(lm, target_modules=targets)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if "lora_B" in n:                                # (the adapters are fp32 modules; the statement copies them to float64)
                p.normal_(0, 0.02, generator=g)
    B, S, H, V = 3, 11, lm.config.hidden_size, lm.config.vocab_size
    emb = torch.randn(B, S, H, generator=g, dtype=torch.float64).requires_grad_(True)
    am = (torch.arange(S)[None] < torch.tensor([11, 7, 4])[:, None]).long()
    labels = torch.randint(0, V, (B, S), generator=g).masked_fill(am == 0, -100)
    labels[:, :2] = -100
    lm.eval()
    ref = R.shifted_ce(lm(inputs_embeds=emb, attention_mask=am)[0], labels)
    ref.backward()
    P = R.llama_params(lm)
    e2 = emb.detach().clone().requires_grad_(True)
    loss = R.shifted_ce(R.llama_logits(lm, P, e2, am), labels)
    loss.backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())          # (the fp32 adapter modules round HF's update; the statement does not)
    assert (e2.grad - emb.grad).abs().max() <= 1e-5 * emb.grad.abs().max()
    n_adapters = 0
    for n, p in lm.named_parameters():
        if "lora_" in n:
            n_adapters += 1
            assert (P[n].grad - p.grad.double()).abs().max() <= 1e-5 * p.grad.abs().max() + 1e-12, n
    assert n_adapters == lm.config.num_hidden_layers * 2 * (2 if targets is None else 7)
