"""Float64 statements of the kernels of csrc/train_llm.hip (forward and the backward formulas the kernels evaluate), of one Llama decoder
layer built from them, and of the whole training forward of ``train.llama_with_grad``.  Plain torch on whatever device the operands are on;
tests/test_train_llm_ref.py proves each against HF's own modules and torch autograd on the CPU, tests/test_gpu_train_llm.py holds the
kernels and the graph to them."""
import math

import torch


# ----------------------------------------------------------------------------- RMSNorm with the residual add in front
def rmsnorm_forward(x, delta, gamma, eps):
    """-> (y, sum, rstd):  sum = x (+ delta),  rstd = rsqrt(mean(sum^2) + eps),  y = gamma * (sum * rstd)."""
    s = x if delta is None else x + delta
    rstd = torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + eps)
    return gamma * (s * rstd), s, rstd


def rmsnorm_backward(dy, s, rstd, gamma, dsum=None):
    """ds = rstd (g . dy) - sum rstd^3 / D  SUM(g . dy . sum)  (+ dsum): the gradient of x and of delta."""
    g = gamma * dy
    ds = rstd * g - s * rstd.pow(3) / s.shape[-1] * (g * s).sum(-1, keepdim=True)
    return ds if dsum is None else ds + dsum


# ----------------------------------------------------------------------------- rotary embedding (rotate-half form)
def rope(x, cos, sin, nh, nkv, hd, conjugate=False):
    """x [B, S, (nh + 2 nkv) hd] = q heads | k heads | v heads; cos / sin [S, hd].  Forward: t cos + rotate_half(t) sin on the q and k heads,
    v copied.  ``conjugate``: the transposed rotation  y1 = c1 x1 + s2 x2,  y2 = c2 x2 - s1 x1."""
    B, S, _ = x.shape
    half = hd // 2
    t = x.reshape(B, S, nh + 2 * nkv, hd)
    rot, keep = t[:, :, : nh + nkv], t[:, :, nh + nkv:]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    x1, x2 = rot[..., :half], rot[..., half:]
    c1, c2, s1, s2 = c[..., :half], c[..., half:], s[..., :half], s[..., half:]
    if not conjugate:
        y = torch.cat([x1 * c1 - x2 * s1, x2 * c2 + x1 * s2], dim=-1)
    else:
        y = torch.cat([x1 * c1 + x2 * s2, x2 * c2 - x1 * s1], dim=-1)
    return torch.cat([y, keep], dim=2).reshape(x.shape)


# ----------------------------------------------------------------------------- SwiGLU
def swiglu_forward(gu):
    I = gu.shape[-1] // 2
    g, u = gu[..., :I], gu[..., I:]
    return g * torch.sigmoid(g) * u


def swiglu_backward(gu, dact):
    I = gu.shape[-1] // 2
    g, u = gu[..., :I], gu[..., I:]
    sig = torch.sigmoid(g)
    return torch.cat([dact * u * sig * (1 + g * (1 - sig)), dact * g * sig], dim=-1)


# ----------------------------------------------------------------------------- causal attention with grouped heads
def _scores(q, k, heads, kv_heads, scale, key_mask, causal=True):
    B, S, _ = q.shape
    hd = q.shape[-1] // heads
    group = heads // kv_heads
    qh = q.reshape(B, S, heads, hd)
    kh = k.reshape(B, S, kv_heads, hd).repeat_interleave(group, dim=2)              # query head h reads K/V head h // group
    s = torch.einsum("bihd,bjhd->bhij", qh, kh) * scale
    if key_mask is not None:
        s = s + key_mask.to(s.dtype)[:, None, None, :]
    if causal:
        above = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(above, -math.inf)
    return s


def attn_causal_forward(q, k, v, heads, kv_heads, scale, key_mask=None, causal=True):
    """q [B, S, heads hd], k / v [B, S, kv_heads hd], key_mask additive [B, S] or None -> (out [B, S, heads hd], lse [B, heads, S])."""
    B, S, _ = q.shape
    hd = q.shape[-1] // heads
    s = _scores(q, k, heads, kv_heads, scale, key_mask, causal)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    vh = v.reshape(B, S, kv_heads, hd).repeat_interleave(heads // kv_heads, dim=2)
    return torch.einsum("bhij,bjhd->bihd", p, vh).reshape(B, S, heads * hd), lse


def attn_causal_backward(q, k, v, out, lse, dout, heads, kv_heads, scale, key_mask=None, causal=True):
    """A = exp(S - lse);  delta_i = dout_i . out_i;  dS = A (dout v^T - delta);  dq = scale dS k;  dk = scale dS^T q and dv = A^T dout summed over
    the query heads of each K/V head."""
    B, S, _ = q.shape
    hd = q.shape[-1] // heads
    group = heads // kv_heads
    A = torch.exp(_scores(q, k, heads, kv_heads, scale, key_mask, causal) - lse[..., None])
    qh, gh, oh = (t.reshape(B, S, heads, hd) for t in (q, dout, out))
    kh = k.reshape(B, S, kv_heads, hd).repeat_interleave(group, dim=2)
    vh = v.reshape(B, S, kv_heads, hd).repeat_interleave(group, dim=2)
    delta = (gh * oh).sum(-1).permute(0, 2, 1)                                       # [B, heads, S]
    dS = A * (torch.einsum("bihd,bjhd->bhij", gh, vh) - delta[..., None])
    dq = torch.einsum("bhij,bjhd->bihd", dS, kh) * scale
    dk = (torch.einsum("bhij,bihd->bjhd", dS, qh) * scale).reshape(B, S, kv_heads, group, hd).sum(3)
    dv = torch.einsum("bhij,bihd->bjhd", A, gh).reshape(B, S, kv_heads, group, hd).sum(3)
    return dq.reshape(q.shape), dk.reshape(k.shape), dv.reshape(v.shape)


# ----------------------------------------------------------------------------- one decoder layer, and the model
def linear(x, w, b=None, lora=None, mask=None):
    """x W^T (+ b) (+ lora_B(lora_A(x * mask)) * scaling);  lora = (A [r, K], B [N, r], scaling)."""
    y = x @ w.t()
    if b is not None:
        y = y + b
    if lora is not None:
        A, Bm, scaling = lora
        xd = x if mask is None else x * mask
        y = y + (xd @ A.t()) @ Bm.t() * scaling
    return y


def llama_layer(x, delta, P, prefix, cos, sin, key_mask, nh, nkv, hd, eps, masks=None):
    """One LlamaDecoderLayer on the residual stream ``x`` and the pending update ``delta`` (None for the first layer) -> (x', delta'): the
    layer's own residual adds are the next norm's.  ``P``: name -> float64 tensor (``<prefix>self_attn.q_proj.weight`` ...; a projection
    with ``.lora_A.default.weight`` carries an adapter, its scaling under ``.scaling``); ``masks``: site -> LoRA dropout mask."""
    masks = masks or {}

    def lin(name, t):
        n = prefix + name
        lora = None
        if n + ".lora_A.default.weight" in P:
            lora = (P[n + ".lora_A.default.weight"], P[n + ".lora_B.default.weight"], P[n + ".scaling"])
        return linear(t, P[n + ".weight"], P.get(n + ".bias"), lora, masks.get(n + ".lora_dropout"))

    h, x, _ = rmsnorm_forward(x, delta, P[prefix + "input_layernorm.weight"], eps)
    qkv = rope(torch.cat([lin("self_attn.q_proj", h), lin("self_attn.k_proj", h), lin("self_attn.v_proj", h)], dim=-1), cos, sin, nh, nkv, hd)
    q, k, v = qkv.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    ctx, _ = attn_causal_forward(q, k, v, nh, nkv, 1.0 / math.sqrt(hd), key_mask)
    delta = lin("self_attn.o_proj", ctx)
    h, x, _ = rmsnorm_forward(x, delta, P[prefix + "post_attention_layernorm.weight"], eps)
    gu = torch.cat([lin("mlp.gate_proj", h), lin("mlp.up_proj", h)], dim=-1)
    return x, lin("mlp.down_proj", swiglu_forward(gu))


def llama_params(lm):
    """name -> float64 copy of every parameter of an HF Llama (adapter parameters as leaves that require grad) + the adapters' scalings."""
    P = {}
    for n, p in lm.named_parameters():
        P[n] = p.detach().double().clone().requires_grad_("lora_" in n)
    for n, m in lm.named_modules():
        if hasattr(m, "lora_A"):
            P[n + ".scaling"] = float(m.scaling)
    return P


def llama_logits(lm, P, inputs_embeds, attention_mask, masks=None):
    """The training forward in float64: logits [B, S, V] from ``inputs_embeds`` [B, S, H] (float64) and a 0 / 1 ``attention_mask`` [B, S]."""
    cfg = lm.config
    nh = cfg.num_attention_heads
    nkv = cfg.num_key_value_heads
    hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // nh
    B, S, _ = inputs_embeds.shape
    rot = lm.model.rotary_emb
    fr = torch.arange(S, dtype=torch.float64, device=inputs_embeds.device)[:, None] * rot.inv_freq.double().to(inputs_embeds.device)[None]
    emb = torch.cat([fr, fr], dim=-1)
    cos, sin = emb.cos() * float(rot.attention_scaling), emb.sin() * float(rot.attention_scaling)
    key_mask = None
    if attention_mask is not None:
        key_mask = torch.zeros(B, S, dtype=torch.float64, device=inputs_embeds.device).masked_fill(attention_mask == 0, torch.finfo(torch.float32).min)
    x, delta = inputs_embeds, None
    for li in range(cfg.num_hidden_layers):
        x, delta = llama_layer(x, delta, P, f"model.layers.{li}.", cos, sin, key_mask, nh, nkv, hd, cfg.rms_norm_eps, masks)
    h, _, _ = rmsnorm_forward(x, delta, P["model.norm.weight"], cfg.rms_norm_eps)
    return h @ P["lm_head.weight"].t()


def shifted_ce(logits, labels):
    V = logits.shape[-1]
    return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
