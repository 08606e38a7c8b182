"""-m gpu: eos-id sets on the fused graph decoders (``eos_sets=True``) under graph replay -- vtgb_llm_pick_greedy in the greedy step,
vtgb_llm_beam_candidates_eos in the beam step.  Fixtures and precision are those of tests/test_gpu_beam_decode.py (the tiny Llama at head_dim
64, lm_head x 40) and tests/test_gpu_t5_beam_decode.py (the tiny T5, lm_head x 4): fp32 ids against HF ``generate`` on the device, token for
token, on the padded batch of 3; at bf16 the decoder against itself -- the set {e, u}, u an id the model never considers, gives exactly the ids
of the single-eos request e (the new kernels against today's path on real bf16 logits).  The eos set of the HF cases is chosen as in
tests/test_eos_sets.py: from HF's eos-free output, two ids that each end a row, one that never occurs, shown on HF alone first."""
import functools

import pytest
import torch

import test_gpu_beam_decode as GL
import test_gpu_t5_beam_decode as GT

pytestmark = pytest.mark.gpu

BEAMS = dict(num_beams=3, repetition_penalty=1.5, length_penalty=1.0)
DK = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def _lm(model, dev, dtype):
    return GL._lm(dev, dtype) if model == "llama" else GT._lm(dev, dtype, DK)


@functools.lru_cache(maxsize=None)
def _decoder(model, dev, dtype, **kw):
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder
    return (GreedyDecoder if model == "llama" else T5GreedyDecoder)(_lm(model, dev, dtype), eos_sets=True, **kw)


def _mod(model):
    return GL if model == "llama" else GT


def _gen(model, ids):
    """The generated ids (a T5's output starts with the decoder start token)."""
    return ids if model == "llama" else ids[:, 1:]


@functools.lru_cache(maxsize=None)
def _hf_cached(model, dev, key):
    M = _mod(model)
    x, m = M._inputs(dev, torch.float32, 3)
    kw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in key}
    return _gen(model, M._hf(_lm(model, dev, torch.float32), x, m, max_new_tokens=M.N_NEW, **kw))


def _hf(model, dev, **kw):
    """HF generate at fp32 on the padded batch of 3 (computed once per request, shared, never written); ``pad_token_id=0`` as in the fixtures."""
    return _hf_cached(model, dev, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))


def _ours(model, dev, dtype=torch.float32, use_graph=True, **kw):
    M = _mod(model)
    x, m = M._inputs(dev, dtype, 3)
    return _gen(model, _decoder(model, dev, dtype).generate(x, M.N_NEW, attention_mask=m, pad_token_id=0, use_graph=use_graph, **kw))


def _enders(out, ids, pad):
    res = []
    for row in out.tolist():
        hit = [j for j, t in enumerate(row) if t in ids]
        j = hit[0] if hit else None
        res.append(row[j] if j is not None and j < len(row) - 1 and all(t == pad for t in row[j + 1:]) else None)
    return res


@functools.lru_cache(maxsize=None)
def _eos_set(model, dev, beams):
    """(e0, e1, u): e0 ends row 0 early, e1 ends another row at another step, u never occurs -- the first such choice from HF's eos-free output
    for which HF alone shows two different ending ids and other ids than the request with e0 alone."""
    kw = dict(BEAMS) if beams else {}
    free = _hf(model, dev, eos_token_id=None, **kw)
    n = free.shape[1]
    V = _lm(model, dev, torch.float32).config.vocab_size
    u = next(v for v in range(V - 1, 0, -1) if v not in free.flatten().tolist())
    for j0 in range(1, n - 1):
        for r in range(1, free.shape[0]):
            for j1 in range(1, n - 1):
                e0, e1 = int(free[0, j0]), int(free[r, j1])
                if j1 == j0 or e0 == e1 or 0 in (e0, e1) or e0 in free[0, :j0].tolist() or e1 in free[r, :j1].tolist():
                    continue
                ids = (e0, e1, u)
                ref = _hf(model, dev, eos_token_id=list(ids), **kw)
                ends = _enders(ref, ids, e0 if beams else 0)
                if ends[0] is None or len({e for e in ends if e is not None}) < 2 or u in ref.flatten().tolist():
                    continue
                if ref.tolist() != _hf(model, dev, eos_token_id=e0, **kw).tolist():
                    return ids
    raise AssertionError("no eos set with two ending ids in HF's output of this fixture")


def _last_state(model, dev, dtype, beams):
    st = next(reversed(_decoder(model, dev, dtype).graphs.values()))
    assert ("beam" in st) == beams and st["graph"] is not None      # the fused step, captured and replayed
    return st


@pytest.mark.parametrize("beams", [False, True], ids=["greedy", "beams"])
@pytest.mark.parametrize("model", ["llama", "t5"])
def test_fp32_ids_equal_hf_generate(dev, model, beams):
    ids = _eos_set(model, dev, beams)
    kw = dict(BEAMS) if beams else {}
    ref = _hf(model, dev, eos_token_id=list(ids), **kw)
    assert len({e for e in _enders(ref, ids, ids[0] if beams else 0) if e is not None}) >= 2      # HF alone: two ids of the set each end a row
    assert ref.tolist() != _hf(model, dev, eos_token_id=ids[0], **kw).tolist()                     # ... and the first id alone gives other ids
    out = _ours(model, dev, eos_token_id=list(ids), **kw)
    st = _last_state(model, dev, torch.float32, beams)
    assert st["eos"] == ids and st["eos_t"].tolist() == list(ids) and st["eos_t"].is_cuda
    assert (st["beam"]["kernel"] if beams else True) and (st["hip"] if model == "t5" else True)
    assert out.tolist() == ref.tolist(), (model, beams, ids)
    if beams:      # the block of min_new_tokens on every id of the set
        kw = dict(kw, min_new_tokens=6)
        ref = _hf(model, dev, eos_token_id=list(ids), **kw)
        assert not any(t in ids for row in ref[:, :6].tolist() for t in row)
        assert _ours(model, dev, eos_token_id=list(ids), **kw).tolist() == ref.tolist()
    else:
        first = [min(j for j, t in enumerate(row) if t in ids) for row in ref.tolist() if any(t in ids for t in row)]
        kw = dict(min_new_tokens=min(first) + 1)      # the earliest hit is blocked
        blocked = _hf(model, dev, eos_token_id=list(ids), **kw)
        assert blocked.tolist() != ref.tolist()
        assert _ours(model, dev, eos_token_id=list(ids), **kw).tolist() == blocked.tolist()


def _torch_pick(logits, step, eos_ids, fin, tok, out, min_new=0, pad=0):
    """``_GraphDecoder._pick``'s greedy branch and ``_emit``'s two writes as torch ops on the device: the statement ops.pick_greedy replaces."""
    if min_new > 0:
        logits = logits.clone()
        blocked = step < min_new
        for e in eos_ids.tolist():
            logits[:, e] = torch.where(blocked, torch.full_like(logits[:, e], float("-inf")), logits[:, e])
    nxt = logits.argmax(-1)
    nxt = torch.where(fin, torch.full_like(nxt, pad), nxt)
    fin.logical_or_(torch.isin(nxt, eos_ids))
    tok.copy_(nxt)
    out.index_copy_(1, step, nxt[:, None])
    return tok


@pytest.mark.parametrize("model", ["llama", "t5"])
def test_bf16_greedy_set_equals_the_single_eos_request(dev, model, monkeypatch):
    """{e, u} against e on the same bf16 decoder: the pick kernel against today's chain of torch ops, on real bf16 logits, under replay."""
    from videotgb_amd import ops
    dec = _decoder(model, dev, torch.bfloat16)
    free = _ours(model, dev, torch.bfloat16, eos_token_id=None)
    V = dec.lm.config.vocab_size
    n = free.shape[1]
    done = 0
    for r, j in ((0, 3), (1, n // 2), (2, n - 3)):
        e = int(free[r, j])
        for min_new in (0, j + 1):
            kw = dict(min_new_tokens=min_new)
            one = _ours(model, dev, torch.bfloat16, eos_token_id=e, **kw)
            st1 = next(reversed(dec.graphs.values()))
            assert st1["eos"] == e and "eos_t" not in st1      # a single id on an eos_sets decoder: today's state, today's path
            # u: an id this request never emits (greedy: the set's run is the same run until it emits e or u, so it never emits u either)
            u = next(v for v in range(V - 1, 0, -1) if v not in free.flatten().tolist() and v not in one.flatten().tolist())
            calls = []
            real = ops.pick_greedy
            monkeypatch.setattr(ops, "pick_greedy", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
            both = _ours(model, dev, torch.bfloat16, eos_token_id=[e, u], **kw)
            swapped = _ours(model, dev, torch.bfloat16, eos_token_id=[u, e], use_graph=False, **kw)
            monkeypatch.setattr(ops, "pick_greedy", real)
            assert calls, "the eos-set state went through ops.pick_greedy"
            assert torch.equal(both, one) and torch.equal(swapped, one), (model, e, u, min_new)
            done += int((one == e).any())
    assert done >= 3, "the chosen ids do end rows"
    # a one-element list and a repeated id: today's state as well
    _ours(model, dev, torch.bfloat16, eos_token_id=[e])
    assert "eos_t" not in next(reversed(dec.graphs.values()))
    _ours(model, dev, torch.bfloat16, eos_token_id=[e, e])
    assert "eos_t" not in next(reversed(dec.graphs.values()))


@pytest.mark.parametrize("model", ["llama", "t5"])
def test_bf16_beam_set_equals_the_single_eos_request(dev, model, monkeypatch):
    """The same with K = 3 beams.  u must never be among the 2K candidates of any step (a candidate that is an eos id changes the search even
    when it is never emitted): the candidates of the single-eos run are recorded on eager steps and u is an id outside them."""
    from videotgb_amd import ops
    dec = _decoder(model, dev, torch.bfloat16)
    V = dec.lm.config.vocab_size
    free = _ours(model, dev, torch.bfloat16, eos_token_id=None, **BEAMS)
    e = next(int(t) for t in free[0, 2:].tolist() if t != 0)
    seen = []
    real = ops.beam_candidates

    def recording(*a, **k):
        sc, ix = real(*a, **k)
        seen.append((ix % V).flatten().clone())
        return sc, ix
    monkeypatch.setattr(ops, "beam_candidates", recording)
    eager = _ours(model, dev, torch.bfloat16, use_graph=False, eos_token_id=e, **BEAMS)
    monkeypatch.setattr(ops, "beam_candidates", real)
    one = _ours(model, dev, torch.bfloat16, eos_token_id=e, **BEAMS)
    st1 = next(reversed(dec.graphs.values()))
    assert "eos_t" not in st1 and st1["eos"] == e and torch.equal(eager, one) and seen
    considered = set(torch.cat(seen).tolist())
    u = next(v for v in range(V - 1, 0, -1) if v not in considered)
    both = _ours(model, dev, torch.bfloat16, eos_token_id=[e, u], **BEAMS)
    st = _last_state(model, dev, torch.bfloat16, True)
    assert st["eos"] == (e, u) and st["beam"]["kernel"]
    assert torch.equal(both, one), (model, e, u)
    assert (one == e).any()
    assert torch.equal(_ours(model, dev, torch.bfloat16, eos_token_id=[e, u], min_new_tokens=5, **BEAMS),
                       _ours(model, dev, torch.bfloat16, eos_token_id=e, min_new_tokens=5, **BEAMS))


def test_the_kernels_run_in_the_step(dev):
    """Eager steps under the profiler: a set launches pick_greedy_kernel (beams: the list instantiation of beam_row_kernel), a single id neither."""
    x, m = GL._inputs(dev, torch.bfloat16, 3)
    dec = _decoder("llama", dev, torch.bfloat16)
    kw = dict(attention_mask=m, pad_token_id=0, use_graph=False)
    _, names = GL._kernel_names(lambda: dec.generate(x, 4, eos_token_id=[5, 6], **kw))
    assert any("pick_greedy_kernel" in k for k in names), names
    _, names = GL._kernel_names(lambda: dec.generate(x, 4, eos_token_id=5, **kw))
    assert not any("pick_greedy_kernel" in k for k in names)
    _, names = GL._kernel_names(lambda: dec.generate(x, 4, eos_token_id=[5, 6], **dict(kw, **BEAMS)))
    assert any("beam_row_kernel" in k and "BeamEosList" in k for k in names), names
    _, names = GL._kernel_names(lambda: dec.generate(x, 4, eos_token_id=5, **dict(kw, **BEAMS)))
    assert any("beam_row_kernel" in k for k in names) and not any("BeamEosList" in k for k in names)


def test_fp8_weights_fp8_cache_and_a_set(dev, monkeypatch):
    """One combination run: decode_weights="fp8", kv_cache="fp8" and a set.  The replayed ids equal that decoder's own eager steps with the
    emission stated in torch ops (``_torch_pick`` in place of the kernel): everything but the emission is the same launches."""
    from videotgb_amd import ops
    dec = _decoder("llama", dev, torch.bfloat16, weights="fp8", kv_cache="fp8")
    x, m = GL._inputs(dev, torch.bfloat16, 3)
    kw = dict(attention_mask=m, pad_token_id=0)
    free = dec.generate(x, GL.N_NEW, eos_token_id=None, **kw)
    ids = [int(free[0, 4]), int(free[2, 9]), next(v for v in range(dec.lm.config.vocab_size - 1, 0, -1) if v not in free.flatten().tolist())]
    out = dec.generate(x, GL.N_NEW, eos_token_id=ids, min_new_tokens=2, **kw)
    st = next(reversed(dec.graphs.values()))
    assert st["attn"] == "split_fp8" and "eos_t" in st and st["graph"] is not None and dec.weights == "fp8"
    monkeypatch.setattr(ops, "pick_greedy", _torch_pick)
    stated = dec.generate(x, GL.N_NEW, eos_token_id=ids, min_new_tokens=2, use_graph=False, **kw)
    assert torch.equal(out, stated), (out.tolist(), stated.tolist())
    assert any(bool((out == i).any()) for i in ids[:2])      # the set does end a row of this run
