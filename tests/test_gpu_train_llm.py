"""The language model's own training pass (opt-in ``train_lm="own"``) on the GPU: the kernels of csrc/train_llm.hip against the float64
statements of tests/train_llm_ref.py (which tests/test_train_llm_ref.py proves against HF's modules), forward and every gradient, under the
bounds tests/test_gpu_train.py holds the existing attention / LayerNorm kernels to; ``train.llama_with_grad`` through ``LoraTrainStep``
against HF's own ``lm(...)`` + autograd; the launch guard; and the default path unchanged."""
import pytest
import torch

import train_llm_ref as R

pytestmark = pytest.mark.gpu

ATTN_TOL = 2e-5                      # test_attention_train_forward_backward_vs_torch_autograd: err <= 2e-5 * max(|want|max, 1e-3)
NORM_Y_TOL, NORM_G_TOL = 2e-6, 5e-6  # test_layernorm_train_forward_backward_vs_torch_autograd: y, and every gradient, of its own max
LOSS_TOL, GRAD_TOL, GRAD_ABS = 1e-5, 1e-4, 1e-10      # test_training_forward_and_prefix_gradients_vs_reference
SEVEN = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need the MI355X"
    return torch.device("cuda")


# ----------------------------------------------------------------------------- kernels
def _key_mask(B, S, kind):
    if kind == "no":
        return None
    m = torch.zeros(B, S)
    if kind == "yes":
        m[-1, S - S // 3:] = torch.finfo(torch.float32).min           # a padded tail, the value llama_with_grad writes
    else:                                                             # "left": the first rows see masked keys only
        m[-1, : S // 3] = torch.finfo(torch.float32).min
    return m


def _attention_case(dev, B, nh, nkv, hd, S, mask):
    from videotgb_amd import train
    g = torch.Generator().manual_seed(B * 1000 + S + nh)
    qkv = torch.randn(B, S, (nh + 2 * nkv) * hd, generator=g)
    go = torch.randn(B, S, nh * hd, generator=g)
    km = _key_mask(B, S, mask)
    x = qkv.to(dev).requires_grad_(True)
    kmd = None if km is None else km.to(dev)
    out = train._HipCausalAttention.apply(x, nh, nkv, hd, hd ** -0.5, kmd)
    out.backward(go.to(dev))
    return qkv, go, km, out.detach(), x.grad.detach()


@pytest.mark.parametrize("B,nh,nkv,hd,S,mask", [(2, 4, 4, 24, 38, "yes"), (1, 8, 2, 128, 130, "no"), (2, 2, 1, 64, 64, "yes"), (1, 2, 2, 16, 65, "no"),
                                               (1, 1, 1, 8, 1, "no")])
def test_causal_attention_forward_backward_vs_float64_statement(dev, B, nh, nkv, hd, S, mask):
    qkv, go, km, out, dqkv = _attention_case(dev, B, nh, nkv, hd, S, mask)
    q, k, v = qkv.double().split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    kmd = None if km is None else km.double()
    want, lse = R.attn_causal_forward(q, k, v, nh, nkv, hd ** -0.5, kmd)
    dq, dk, dv = R.attn_causal_backward(q, k, v, want, lse, go.double(), nh, nkv, hd ** -0.5, kmd)
    gq, gk, gv = dqkv.cpu().double().split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    for name, got, ref in (("out", out.cpu().double(), want), ("dq", gq, dq), ("dk", gk, dk), ("dv", gv, dv)):
        err = (got - ref).abs().max().item()
        print(f"[causal attention {B, nh, nkv, hd, S, mask}] {name}: max|diff| {err:.3e} of {ref.abs().max().item():.3e}")
        assert err <= ATTN_TOL * max(ref.abs().max().item(), 1e-3), (name, err)
    out2, dqkv2 = _attention_case(dev, B, nh, nkv, hd, S, mask)[3:]
    assert torch.equal(out, out2) and torch.equal(dqkv, dqkv2)        # fixed summation order, no atomics: the same bits


def test_causal_attention_rows_without_a_visible_key_stay_finite(dev):
    B, nh, nkv, hd, S = 2, 4, 2, 32, 70
    qkv, go, km, out, dqkv = _attention_case(dev, B, nh, nkv, hd, S, "left")
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
    # the rows that do see a key agree with the statement (the masked-only rows are padding: whatever finite value)
    q, k, v = qkv.double().split([nh * hd, nkv * hd, nkv * hd], dim=-1)
    want, _ = R.attn_causal_forward(q, k, v, nh, nkv, hd ** -0.5, km.double())
    err = (out.cpu().double() - want)[:, S // 3:].abs().max().item()
    assert err <= ATTN_TOL * max(want.abs().max().item(), 1e-3), err


def test_causal_entry_agrees_with_the_non_causal_entry_on_the_causal_keys(dev):
    """kv_heads == heads, with a key mask: row i of the causal launch is the existing vtgb_attn_train_forward run on query i over keys 0 .. i."""
    from videotgb_amd import train
    B, H, hd, S = 2, 4, 24, 70
    qkv, _, km, out, _ = _attention_case(dev, B, H, H, hd, S, "yes")
    q, k, v = (t.contiguous().to(dev) for t in qkv.split([H * hd] * 3, dim=-1))
    want, _ = R.attn_causal_forward(*qkv.double().split([H * hd] * 3, dim=-1), H, H, hd ** -0.5, km.double())
    for i in (0, 1, 37, 63, 64, S - 1):
        row = train._HipAttention.apply(q[:, i:i + 1], k[:, : i + 1], v[:, : i + 1], H, hd ** -0.5, km[:, : i + 1].to(dev), None)
        bound = ATTN_TOL * max(want[:, i].abs().max().item(), 1e-3)
        assert (row[:, 0] - out[:, i]).abs().max().item() <= 2 * bound, i          # each within `bound` of the statement
        assert (row[:, 0].cpu().double() - want[:, i]).abs().max().item() <= bound, i


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("D", [32, 4096, 8192])
@pytest.mark.parametrize("use_delta", [False, True])
def test_rmsnorm_forward_backward_vs_float64_statement(dev, rows, D, use_delta):
    from videotgb_amd import train
    g = torch.Generator().manual_seed(D + rows)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(dev).requires_grad_(True)
    delta = torch.randn(rows, D, generator=g).to(dev).requires_grad_(True) if use_delta else None
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    w, w2 = torch.randn(rows, D, generator=g).to(dev), torch.randn(rows, D, generator=g).to(dev)

    def run():
        for t in (x, delta):
            if t is not None:
                t.grad = None
        y, s = train.rms_norm(x, gamma, 1e-6, delta)
        ((y * w).sum() + (s * w2).sum()).backward()              # the residual stream's later consumers hand w2 back: the kernel's dsum
        return y.detach(), s.detach(), x.grad.clone(), None if delta is None else delta.grad.clone()

    y, s, gx, gd = run()
    y64, s64, rstd = R.rmsnorm_forward(x.detach().double(), None if delta is None else delta.detach().double(), gamma.double(), 1e-6)
    ds = R.rmsnorm_backward(w.double(), s64, rstd, gamma.double(), dsum=w2.double())
    assert torch.equal(s, x.detach() + delta.detach() if use_delta else x.detach())
    ey, eg = (y.double() - y64).abs().max().item(), (gx.double() - ds).abs().max().item()
    print(f"[rmsnorm rows={rows} D={D} delta={use_delta}] y {ey:.3e} of {y64.abs().max().item():.3e}; ds {eg:.3e} of {ds.abs().max().item():.3e}")
    assert ey <= NORM_Y_TOL * y64.abs().max()
    assert eg <= NORM_G_TOL * ds.abs().max()
    if use_delta:
        assert torch.equal(gd, gx)                               # one gradient for x and delta
    again = run()
    assert torch.equal(y, again[0]) and torch.equal(gx, again[2])


def test_rmsnorm_node_refuses_a_trainable_weight(dev):
    from videotgb_amd import train
    with pytest.raises(NotImplementedError, match="trainable RMSNorm weight"):
        train.rms_norm(torch.randn(2, 32, device=dev), torch.ones(32, device=dev, requires_grad=True), 1e-6)


def _tables(S, hd, dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    fr = torch.arange(S, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat([fr, fr], dim=-1)
    return emb.cos().to(dev), emb.sin().to(dev)


@pytest.mark.parametrize("hd", [16, 64, 128])
@pytest.mark.parametrize("nh,nkv", [(2, 2), (8, 2)])
def test_rope_forward_conjugate_vs_float64_statement(dev, hd, nh, nkv):
    from videotgb_amd import train
    B, S = 2, 5
    g = torch.Generator().manual_seed(hd + nh)
    cos, sin = _tables(S, hd, dev)
    x = torch.randn(B, S, (nh + 2 * nkv) * hd, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(x.shape, generator=g).to(dev)
    y = train._HipRope.apply(x, cos, sin, nh, nkv, hd)
    y.backward(w)
    want = R.rope(x.detach().double(), cos.double(), sin.double(), nh, nkv, hd)
    dx = R.rope(w.double(), cos.double(), sin.double(), nh, nkv, hd, conjugate=True)
    assert (y.detach().double() - want).abs().max() <= NORM_Y_TOL * want.abs().max()
    assert (x.grad.double() - dx).abs().max() <= NORM_G_TOL * dx.abs().max()
    assert torch.equal(y.detach()[..., (nh + nkv) * hd:], x.detach()[..., (nh + nkv) * hd:])      # v passes through
    back = train._HipRope._run(y.detach().contiguous(), cos, sin, nh, nkv, hd, 1)                 # conjugate(forward(x)) == x to rounding
    assert (back - x.detach()).abs().max() <= NORM_Y_TOL * x.detach().abs().max()
    # a table whose two halves differ: the conjugate is still the transpose
    c2, s2 = torch.randn(S, hd, generator=g).to(dev), torch.randn(S, hd, generator=g).to(dev)
    got = train._HipRope._run(w, c2, s2, nh, nkv, hd, 1)
    ref = R.rope(w.double(), c2.double(), s2.double(), nh, nkv, hd, conjugate=True)
    assert (got.double() - ref).abs().max() <= NORM_G_TOL * ref.abs().max()


@pytest.mark.parametrize("M,I", [(1, 64), (67, 11008)])
def test_swiglu_forward_backward_vs_float64_statement(dev, M, I):
    from videotgb_amd import train
    g = torch.Generator().manual_seed(M + I)
    gu = (torch.randn(M, 2 * I, generator=g) * 3).to(dev).requires_grad_(True)
    w = torch.randn(M, I, generator=g).to(dev)
    act = train._HipSwiGlu.apply(gu)
    act.backward(w)
    want = R.swiglu_forward(gu.detach().double())
    dgu = R.swiglu_backward(gu.detach().double(), w.double())
    assert (act.detach().double() - want).abs().max() <= NORM_Y_TOL * want.abs().max()
    assert (gu.grad.double() - dgu).abs().max() <= NORM_G_TOL * dgu.abs().max()


# ----------------------------------------------------------------------------- the graph, through LoraTrainStep
class _Holder:                                                   # the attribute layout LoraTrainStep expects of an LSTP twin
    def __init__(self, lm):
        self.model = type("M", (), {})()
        self.model.language_model = lm


def _batch(lm, dev):
    """The ragged batch of test_lora_micro_step_matches_plain_pytorch."""
    g = torch.Generator().manual_seed(5)
    B, P, Li, Lo, H, V = 3, 4, 6, 5, lm.config.hidden_size, lm.config.vocab_size
    prefix = torch.randn(B, P, H, generator=g).to(dev)
    qlen, alen = torch.tensor([6, 3, 1]), torch.tensor([5, 2, 4])
    q_att = (torch.arange(Li)[None] < qlen[:, None]).long()
    a_att = (torch.arange(Lo)[None] < alen[:, None]).long()
    q = torch.randint(3, V, (B, Li), generator=g) * q_att
    a = torch.randint(3, V, (B, Lo), generator=g) * a_att
    return prefix, q.to(dev), q_att.to(dev), a.to(dev), a_att.to(dev)


def _step(dev, kv_heads=2, targets=None, train_lm="own", **kw):
    from videotgb_amd import llm, train
    lm = llm.build_llama("tiny", torch.float32, dev, num_key_value_heads=kv_heads)
    step = train.LoraTrainStep(_Holder(lm), pad_token_id=0, lr=1e-2, accumulate_grad_batches=4, train_prefix=False, train_lm=train_lm,
                               lora_target_modules=targets, **kw)
    lm.eval()
    g = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if "lora_A" in n:                                    # LoraLinear draws A from the global generator: whatever ran before would
                bound = 1.0 / p.shape[1] ** 0.5                  # decide this test's inputs.  kaiming_uniform_(a=sqrt(5)): U(-1/sqrt(fan_in), +)
                p.uniform_(-bound, bound, generator=g)
            if "lora_B" in n:
                p.normal_(0, 0.02, generator=g)
    return step, lm


def _own(step, lm, batch):
    """loss and gradients (adapters by name, and the prefix) of one own-kernel micro-batch."""
    prefix = batch[0].detach().clone().requires_grad_(True)
    lm.zero_grad()
    loss = step.loss(prefix, *batch[1:])
    loss.backward()
    grads = {n: p.grad.clone() for n, p in lm.named_parameters() if p.requires_grad}
    grads["prefix"] = prefix.grad.clone()
    lm.zero_grad()
    return loss.detach(), grads


def _hf(lm, batch, autocast=False):
    """HF's own lm(...) + the oracle's shifted CE + backward on the same micro-batch."""
    from oracle import vtgb_oracle as O
    prefix, q, q_att, a, a_att = batch
    prefix = prefix.detach().clone().requires_grad_(True)
    toks, lens = O.concat_text_input_output(q.cpu(), q_att.cpu(), a.cpu(), a_att.cpu())
    labels = O.lm_labels(toks["input_ids"], lens, 0, prefix.shape[1]).to(prefix.device)
    emb = lm.get_input_embeddings()(toks["input_ids"].to(prefix.device))
    am = torch.cat([torch.ones(prefix.shape[:2], dtype=torch.long), toks["attention_mask"]], 1).to(prefix.device)
    lm.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = lm(inputs_embeds=torch.cat([prefix, emb], 1), attention_mask=am)[0]
    loss = O.shifted_cross_entropy(logits.float(), labels)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in lm.named_parameters() if p.requires_grad}
    grads["prefix"] = prefix.grad.clone()
    lm.zero_grad()
    return loss.detach(), grads


def _assert_close(tag, loss, grads, ref_loss, ref_grads, want_names):
    print(f"[{tag}] loss {loss.item():.7f} vs {ref_loss.item():.7f}")
    assert abs(loss.item() - ref_loss.item()) <= LOSS_TOL * abs(ref_loss.item())
    assert set(grads) == set(want_names) | {"prefix"}
    worst = 0.0
    for n, want in ref_grads.items():
        err, scale = (grads[n].double() - want.double()).abs().max().item(), want.abs().max().item()
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= GRAD_TOL * scale + GRAD_ABS, (n, err, scale)
    print(f"[{tag}] {len(ref_grads)} gradient tensors, worst max|diff| / max|ref| = {worst:.2e}")


@pytest.mark.parametrize("kv_heads,targets", [(2, None), (1, None), (2, SEVEN)])
def test_own_training_pass_matches_hf_forward_and_autograd(dev, kv_heads, targets):
    step, lm = _step(dev, kv_heads, targets)
    batch = _batch(lm, dev)
    names = [n for n, _ in lm.named_parameters() if "lora_" in n]
    assert len(names) == lm.config.num_hidden_layers * 2 * (2 if targets is None else 7)
    loss, grads = _own(step, lm, batch)
    ref_loss, ref_grads = _hf(lm, batch)
    _assert_close(f"own vs HF kv={kv_heads} targets={'default' if targets is None else 'seven'}", loss, grads, ref_loss, ref_grads, names)
    assert step.drawn == {}                                      # eval mode: no dropout site drew


def _statement(lm, batch, masks):
    """Loss and gradients of the float64 model statement on the micro-batch, LoRA dropout masks injected."""
    from videotgb_amd import train
    prefix, q, q_att, a, a_att = batch
    toks, _, labels = train.concat_text_input_output(q, q_att, a, a_att, 0, prefix.shape[1])
    emb = lm.get_input_embeddings()(toks["input_ids"]).detach()
    x = torch.cat([prefix, emb], 1).double().requires_grad_(True)
    am = torch.cat([torch.ones(prefix.shape[:2], dtype=torch.long, device=prefix.device), toks["attention_mask"]], 1)
    P = R.llama_params(lm)
    loss = R.shifted_ce(R.llama_logits(lm, P, x, am, {k: v.double() for k, v in masks.items()}), labels)
    loss.backward()
    grads = {n: P[n].grad for n, p in lm.named_parameters() if p.requires_grad}
    grads["prefix"] = x.grad[:, : prefix.shape[1]]
    return loss.detach(), grads


def test_lora_dropout_masks_are_recorded_replayed_bit_for_bit_and_match_the_statement(dev):
    from videotgb_amd import train
    step, lm = _step(dev)
    batch = _batch(lm, dev)
    lm.train()                                                   # LoRA dropout 0.1 (apply_lora's default)
    step.dropout_generator = torch.Generator(device=dev).manual_seed(11)
    loss1, g1 = _own(step, lm, batch)
    drawn = dict(step.drawn)
    sites = {f"model.layers.{i}.self_attn.{p}.lora_dropout" for i in range(lm.config.num_hidden_layers) for p in ("q_proj", "v_proj")}
    assert set(drawn) == sites
    keep = torch.tensor(1.0 / 0.9).item()
    for m in drawn.values():
        vals = set(torch.unique(m).tolist())
        assert vals <= {0.0, keep} and vals == {0.0, keep}, sorted(vals)[:4]
    loss_other, _ = _own(step, lm, batch)                        # fresh masks: another loss
    assert loss_other.item() != loss1.item()
    step.lm_dropout = train.Dropout(0.1, masks=drawn)
    loss2, g2 = _own(step, lm, batch)
    assert torch.equal(loss1, loss2) and set(step.drawn) == sites
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    ref_loss, ref_grads = _statement(lm, batch, drawn)
    _assert_close("own (train mode, masks injected) vs float64 statement", loss1, g1, ref_loss, ref_grads, [n for n in g1 if n != "prefix"])


def _rel_rms(a, b):
    return ((a.double() - b.double()).pow(2).sum().sqrt() / b.double().pow(2).sum().sqrt().clamp_min(1e-30)).item()


def _token_losses(lm, batch, mode):
    """(logits [B, S, V] fp32, the loss of every label position [n]) of the micro-batch: "fp32" / "autocast" = HF's lm(...), "own" = llama_with_grad
    with bf16 GEMM operands.  The mean of the second is the step's loss."""
    from videotgb_amd import train
    prefix, q, q_att, a, a_att = batch
    toks, _, labels = train.concat_text_input_output(q, q_att, a, a_att, 0, prefix.shape[1])
    x = torch.cat([prefix, lm.get_input_embeddings()(toks["input_ids"])], 1)
    am = torch.cat([torch.ones(prefix.shape[:2], dtype=torch.long, device=prefix.device), toks["attention_mask"]], 1)
    with torch.no_grad():
        if mode == "own":
            logits = train.llama_with_grad(lm, x, am, "bf16")
        else:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "autocast"):
                logits = lm(inputs_embeds=x, attention_mask=am)[0]
    logits = logits.float()
    V = logits.shape[-1]
    tgt = labels[:, 1:].reshape(-1)
    per = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), tgt, ignore_index=-100, reduction="none")
    return logits, per[tgt != -100]


def test_bf16_compute_is_no_further_from_hf_fp32_than_hf_autocast(dev):
    """Three-way, as tests/test_gpu_stages.py does for ViT-g: HF fp32 is the reference, HF under autocast(bfloat16) sets the distance a bf16 pass
    may have, the own pass with bf16 GEMM operands must be within 1.25 x of it, per tensor, in rel-RMS: every gradient tensor, the logits, and
    the loss.  The loss enters as the tensor it is the mean of -- one value per label position -- so that its distance is a rel-RMS over the
    batch's label positions like the others, not the ratio of two single rounding-error samples (the scalars' distances are printed)."""
    step, lm = _step(dev, lm_compute_dtype="bf16")
    batch = _batch(lm, dev)
    ref_loss, ref = _hf(lm, batch)
    ac_loss, ac = _hf(lm, batch, autocast=True)
    loss, own = _own(step, lm, batch)
    d_ac, d_own = abs(ac_loss.item() - ref_loss.item()) / abs(ref_loss.item()), abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    print(f"[bf16 three-way] mean loss: HF autocast {d_ac:.3e}, own bf16 {d_own:.3e} from HF fp32 (relative)")
    (lg_ref, tl_ref), (lg_ac, tl_ac), (lg_own, tl_own) = (_token_losses(lm, batch, m) for m in ("fp32", "autocast", "own"))
    assert tl_ref.numel() >= 8 and abs(tl_ref.mean().item() - ref_loss.item()) <= 1e-5 * abs(ref_loss.item())      # the loss IS this tensor's mean
    assert abs(tl_own.mean().item() - loss.item()) <= 1e-5 * abs(loss.item())
    rows = [("loss per label position", _rel_rms(tl_ac, tl_ref), _rel_rms(tl_own, tl_ref)), ("logits", _rel_rms(lg_ac, lg_ref), _rel_rms(lg_own, lg_ref))]
    for n in ref:
        rows.append((n, _rel_rms(ac[n], ref[n]), _rel_rms(own[n], ref[n])))
    for n, a, o in rows:
        print(f"[bf16 three-way] {n}: HF autocast {a:.3e}, own bf16 {o:.3e} from HF fp32 (rel-RMS)")
    for n, a, o in rows:
        assert o <= 1.25 * a, (n, o, a)


def test_a_stated_model_is_still_guarded_on_later_calls(dev):
    """The full ``llama_train_state`` walk runs on a model's first call only; what a later call reads is checked where it is read."""
    step, lm = _step(dev)
    batch = _batch(lm, dev)
    _own(step, lm, batch)
    w = lm.model.layers[1].mlp.down_proj.weight
    w.requires_grad = True
    with pytest.raises(NotImplementedError, match="model.layers.1.mlp.down_proj.weight: a trainable parameter"):
        step.loss(*batch)
    w.requires_grad = False
    lm.model.norm.weight.requires_grad = True
    with pytest.raises(NotImplementedError, match="trainable RMSNorm weight"):
        step.loss(*batch)


# ----------------------------------------------------------------------------- launch guard, default path, optimizer step
NEW_KERNELS = ("rmsnorm_train_fwd_kernel", "rmsnorm_train_bwd_kernel", "rope_train_kernel", "swiglu_train_fwd_kernel", "swiglu_train_bwd_kernel",
               "attn_causal_fwd_kernel", "attn_causal_dq_kernel", "attn_causal_dkv_kernel")


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() if e.device_time_total > 0]


@pytest.mark.parametrize("code", ["f32", "bf16"])
def test_own_pass_launches_no_blas_and_no_torch_llm_kernel(dev, code):
    """One loss(...).backward() under train_lm="own": every GEMM is the library's, the new kernels run, and nothing of HF's Llama is launched --
    no hipBLASLt / rocBLAS kernel (Cijk_*), no SDPA / softmax, no silu, no RMS-norm elementwise chain (pow / rsqrt)."""
    step, lm = _step(dev, lm_compute_dtype=code)
    batch = _batch(lm, dev)
    lm.train()
    names = _kernel_names(lambda: _own(step, lm, batch))
    for k in NEW_KERNELS:
        assert any(k in n for n in names), (k, names)
    assert any("tg_mfma_kernel" in n or "tg_f32_kernel" in n for n in names), names
    low = [n.lower() for n in names]
    bad = [n for n in low if "cijk_" in n or "softmax" in n or "silu" in n or "rsqrt" in n or "pow_tensor" in n or "fmha" in n or "flash" in n
           or "attention" in n or "sdpa" in n]
    assert not bad, bad


def test_default_path_is_hf_and_launches_none_of_the_new_kernels(dev):
    from videotgb_amd import train
    for kw in ({}, dict(train_lm="hf")):
        from videotgb_amd import llm
        lm = llm.build_llama("tiny", torch.float32, dev)
        step = train.LoraTrainStep(_Holder(lm), pad_token_id=0, train_prefix=False, **kw)
        assert step.train_lm == "hf"
        calls = []
        h = lm.register_forward_hook(lambda *a: calls.append(1))
        batch = _batch(lm, dev)
        names = _kernel_names(lambda: step.loss(*batch).backward())
        h.remove()
        assert len(calls) == 2                                   # one lm.forward per loss (the warm-up call and the profiled one)
        assert not [n for n in names if any(k in n for k in NEW_KERNELS)]


def test_interface_refusals_on_the_device(dev):
    from videotgb_amd import llm, train
    with pytest.raises(ValueError, match="train_lm='x'"):
        train.LoraTrainStep(_Holder(llm.build_llama("tiny", torch.float32, dev)), 0, train_prefix=False, train_lm="x")
    with pytest.raises(NotImplementedError, match="attention_dropout 0.1"):
        train.LoraTrainStep(_Holder(llm.build_llama("tiny", torch.float32, dev, attention_dropout=0.1)), 0, train_prefix=False, train_lm="own")
    from transformers import T5Config, T5ForConditionalGeneration
    t5 = T5ForConditionalGeneration(T5Config(vocab_size=64, d_model=16, d_kv=8, d_ff=32, num_layers=1, num_heads=2)).to(dev)
    with pytest.raises(NotImplementedError, match="Llama language model only"):
        train.LoraTrainStep(_Holder(t5), 0, train_prefix=False, train_lm="own")


def test_one_optimizer_step_moves_the_adapters_and_nothing_else(dev):
    step, lm = _step(dev)
    batch = _batch(lm, dev)
    lm.zero_grad()
    before = {n: p.detach().clone() for n, p in lm.named_parameters()}
    flags = [step.step(*batch)[1] for _ in range(4)]
    assert flags == [False, False, False, True]
    for n, p in lm.named_parameters():
        assert ("lora_" in n) == (not torch.equal(before[n], p.detach())), n


def test_live_parameters_are_seen_by_the_next_call(dev):
    step, lm = _step(dev)
    batch = _batch(lm, dev)
    l0, _ = _own(step, lm, batch)
    with torch.no_grad():
        lm.model.layers[0].self_attn.q_proj.lora_B["default"].weight.mul_(3.0)
    l1, _ = _own(step, lm, batch)
    assert l0.item() != l1.item()


# ----------------------------------------------------------------------------- the LightningModule twins
def _twin(dev, tmp_path, cls_name, arch, llm, **kw):
    import functools
    from conftest import full_state_dict, write_hf_config
    from videotgb_amd import models, modules
    from videotgb_amd.synth import tiny_cfg
    cfg = tiny_cfg(arch)
    base = write_hf_config(str(tmp_path / f"{arch}-tiny"), arch, cfg, llm)
    sd = full_state_dict(cfg, models.build_language_model(models.load_hf_config(base, arch)))
    raft_pth = str(tmp_path / "raft-things.pth")
    torch.save({"module." + k[len("of_extractor."):]: v for k, v in sd.items() if k.startswith("of_extractor.")}, raft_pth)
    proc = type("P", (), dict(tokenizer=type("T", (), dict(pad_token_id=0))()))()
    m = getattr(modules, cls_name)(model_name_or_path=base, sampler_name_or_path=str(tmp_path / "no-bert-weights"), of_extractor_name_or_path=raft_pth,
                                   temperature=1.0, optimizer=functools.partial(torch.optim.AdamW, lr=1e-4), scheduler="cosine",
                                   scheduler_params={"warmup_steps": 0.1}, generate_configs=dict(do_sample=False, max_new_tokens=6),
                                   compute_dtype="f32", processor=proc, tgb_cfg=cfg.tgb, **kw)
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def test_twin_forward_takes_its_logits_from_the_own_graph(dev, tmp_path):
    """LSTPModule(train_lm="own").forward against the same twin with the switch back on "hf": loss, logits and the gradient that reaches the
    Q-Former through the language model; and no lm.forward call under "own"."""
    from conftest import load_golden
    from test_gpu_modules import up4
    m = _twin(dev, tmp_path, "LSTPModule", "instructblip", "llama", train_lm="own")
    assert m.train_lm == "own"
    m.eval()
    g = load_golden("tiny_modules")
    B = 2
    batch = dict(frames=(up4(g["frames_q8"]) / 48).to(dev), nframe=int(g["nframe"]), of_lengths=g["of_lengths"].tolist(),
                 sampler_question=g["ib_sampler_ids"].to(dev), sampler_question_attention_mask=g["ib_sampler_mask"].to(dev),
                 qformer_text=g["ib_qformer_ids"].to(dev), qformer_text_attention_mask=g["ib_qformer_mask"].to(dev),
                 question=g["ib_question"].to(dev), question_attention_mask=g["ib_question_mask"].to(dev),
                 answer=torch.randint(3, 100, (B, 4), generator=torch.Generator().manual_seed(1)).to(dev),
                 answer_attention_mask=torch.ones(B, 4, dtype=torch.long, device=dev),
                 of=(up4(g["of_q8"]) / 127).to(dev)[:, :8], of_mask=torch.ones(B, 10, dtype=torch.long, device=dev))
    noise = g["ib_noise"].to(dev) if "ib_noise" in g else None
    calls = []
    h = m.model.language_model.register_forward_hook(lambda *a: calls.append(1))
    out = {}
    for leg in ("own", "hf"):
        m.train_lm = leg
        m.zero_grad()
        loss, logits = m.forward(batch, noise=noise)
        loss.backward()
        out[leg] = (loss.detach(), logits.detach().float(), m.model.query_tokens.grad.clone(), len(calls))
    h.remove()
    assert out["own"][3] == 0 and out["hf"][3] == 1
    assert abs(out["own"][0].item() - out["hf"][0].item()) <= LOSS_TOL * abs(out["hf"][0].item())
    for i in (1, 2):
        err, scale = (out["own"][i] - out["hf"][i]).abs().max().item(), out["hf"][i].abs().max().item()
        assert scale > 0 and err <= GRAD_TOL * scale + GRAD_ABS, (i, err, scale)


def test_seq2seq_twin_refuses_the_own_pass(dev, tmp_path):
    with pytest.raises(NotImplementedError, match="Llama language model only"):
        _twin(dev, tmp_path, "LSTPBlip2Module", "blip2", "t5", train_lm="own")
    with pytest.raises(ValueError, match="train_lm='x'"):
        _twin(dev, tmp_path, "LSTPBlip2Module", "blip2", "t5", train_lm="x")
