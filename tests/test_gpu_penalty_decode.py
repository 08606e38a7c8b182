"""-m gpu: a repetition penalty on ONE beam on the fused graph decoders (``penalty=True``) under graph replay -- vtgb_llm_repetition_penalty in
front of the emission of the captured step.  Fixtures are those of tests/test_gpu_beam_decode.py (the tiny Llama at head_dim 64, lm_head x 40)
and tests/test_gpu_t5_beam_decode.py (the tiny T5 at d_kv 64, lm_head x 4), on the padded batch of 3 with p = 1.5: fp32 ids against HF
``generate`` on the device, token for token (shown on HF alone first: every row's penalised ids differ from its unpenalised ones); at bf16
the kernel decoder against the same decoder with ``PENALTY_KERNEL = False`` (the torch statement on real bf16 logits)."""
import functools
import types

import pytest
import torch

import test_gpu_beam_decode as GL
import test_gpu_t5_beam_decode as GT

pytestmark = pytest.mark.gpu

P_, DK = 1.5, 64
MODELS = ("llama", "t5")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def _mod(model):
    return GL if model == "llama" else GT


def _lm(model, dev, dtype):
    return GL._lm(dev, dtype) if model == "llama" else GT._lm(dev, dtype, DK)


def _decoder(model, dev, dtype, kernel=True):
    return _decoder_cached(model, dev, dtype, bool(kernel))      # (one object per combination, however the arguments are given)


@functools.lru_cache(maxsize=None)
def _decoder_cached(model, dev, dtype, kernel):
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder
    dec = (GreedyDecoder if model == "llama" else T5GreedyDecoder)(_lm(model, dev, dtype), penalty=True)
    if not kernel:
        dec.PENALTY_KERNEL = False      # the class switch, on this object: the fused path runs the torch statement
    return dec


def _gen(model, ids):
    """The generated ids (a T5's output starts with the decoder start token)."""
    return ids if model == "llama" else ids[:, 1:]


@functools.lru_cache(maxsize=None)
def _hf_cached(model, dev, key):
    M = _mod(model)
    x, m = M._inputs(dev, torch.float32, 3)
    return _gen(model, M._hf(_lm(model, dev, torch.float32), x, m, max_new_tokens=M.N_NEW, **dict(key)))


def _hf(model, dev, **kw):
    """HF generate at fp32 on the padded batch of 3 (computed once per request, shared, never written); ``pad_token_id=0`` as in the fixtures."""
    return _hf_cached(model, dev, tuple(sorted(kw.items())))


def _ours(model, dev, dtype=torch.float32, kernel=True, use_graph=True, **kw):
    M = _mod(model)
    x, m = M._inputs(dev, dtype, 3)
    return _gen(model, _decoder(model, dev, dtype, kernel).generate(x, M.N_NEW, attention_mask=m, pad_token_id=0, use_graph=use_graph, **kw))


def _rows_differ(a, b):
    n = min(a.shape[1], b.shape[1])
    return all(bool((a[r, :n] != b[r, :n]).any()) for r in range(a.shape[0]))


@functools.lru_cache(maxsize=None)
def _eos(model, dev):
    """An eos id from HF's own penalised eos-free output with which HF ends one row early (the rest pad), leaves another running to the
    last column, and still gives every row other ids than without the penalty."""
    free, plain = _hf(model, dev, repetition_penalty=P_, eos_token_id=None), _hf(model, dev, eos_token_id=None)
    n = free.shape[1]
    for j in range(1, n - 1):
        for r in range(free.shape[0]):
            e = int(free[r, j])
            # (cheap, on the eos-free outputs, before HF runs again: the id first occurs here, after the penalty has changed the row, and another row never emits it)
            if e == 0 or e in free[r, :j].tolist() or not (free[r, :j + 1] != plain[r, :j + 1]).any() or all(e in row for row in free.tolist()):
                continue
            ref = _hf(model, dev, repetition_penalty=P_, eos_token_id=e)
            row = ref[r].tolist()
            early = e in row and row.index(e) == j and all(t == 0 for t in row[j + 1:])
            full = ref.shape[1] == n and any(e not in other for other in ref.tolist())
            if early and full and _rows_differ(ref, _hf(model, dev, eos_token_id=e)):
                return e
    raise AssertionError("no eos id that ends one row early and leaves one running in HF's penalised output of this fixture")


def _last_state(model, dev, dtype, kernel=True):
    st = next(reversed(_decoder(model, dev, dtype, kernel).graphs.values()))
    assert st["graph"] is not None and "beam" not in st and (st["hip"] if model == "t5" else True)      # the fused step, captured and replayed
    return st


@pytest.mark.parametrize("model", MODELS)
def test_fp32_ids_equal_hf_generate(dev, model):
    for eos in (None, _eos(model, dev)):
        ref = _hf(model, dev, repetition_penalty=P_, eos_token_id=eos)
        assert _rows_differ(ref, _hf(model, dev, eos_token_id=eos)), (model, eos)      # HF alone: the penalty decides ids in every row
        out = _ours(model, dev, repetition_penalty=P_, eos_token_id=eos)
        st = _last_state(model, dev, torch.float32)
        assert st["pen"] == P_ and st["pen_out"].shape == (3, _lm(model, dev, torch.float32).config.vocab_size) and st["pen_out"].dtype == torch.float32
        assert out.tolist() == ref.tolist(), (model, eos)
    e = _eos(model, dev)
    assert (ref == e).any() and any(e not in row for row in ref.tolist())


@pytest.mark.parametrize("model", MODELS)
def test_bf16_kernel_ids_equal_the_statements(dev, model):
    """The same bf16 decoder with the kernel and with ``PENALTY_KERNEL = False``: the same ids, under replay and on eager steps."""
    plain = _ours(model, dev, torch.bfloat16, eos_token_id=None)
    kern = _ours(model, dev, torch.bfloat16, repetition_penalty=P_, eos_token_id=None)
    assert "pen_out" in _last_state(model, dev, torch.bfloat16)
    stmt = _ours(model, dev, torch.bfloat16, kernel=False, repetition_penalty=P_, eos_token_id=None)
    _last_state(model, dev, torch.bfloat16, kernel=False)
    assert torch.equal(kern, stmt), (model, kern.tolist(), stmt.tolist())
    assert _rows_differ(kern, plain)      # the penalty decides ids here too
    assert torch.equal(_ours(model, dev, torch.bfloat16, use_graph=False, repetition_penalty=P_, eos_token_id=None), kern)
    e = int(kern[0, 4])
    kw = dict(repetition_penalty=P_, eos_token_id=e, min_new_tokens=2)
    assert torch.equal(_ours(model, dev, torch.bfloat16, **kw), _ours(model, dev, torch.bfloat16, kernel=False, **kw))


@pytest.mark.parametrize("model", MODELS)
def test_the_cached_state_is_reused_and_another_penalty_is_another_state(dev, model):
    dec = _decoder(model, dev, torch.float32)
    a = _ours(model, dev, repetition_penalty=P_, eos_token_id=None)
    st = _last_state(model, dev, torch.float32)
    graph = st["graph"]
    b = _ours(model, dev, repetition_penalty=P_, eos_token_id=None)
    assert next(reversed(dec.graphs.values())) is st and st["graph"] is graph and torch.equal(a, b)      # the second call: the same state, the same graph
    _ours(model, dev, repetition_penalty=0.7, eos_token_id=None)
    other = _last_state(model, dev, torch.float32)
    assert other is not st and other["pen"] == 0.7 and other["pen_out"].data_ptr() != st["pen_out"].data_ptr()
    keys = list(dec.graphs)
    assert ("penalty", P_) in keys[-2] and ("penalty", 0.7) in keys[-1]
    c = _ours(model, dev, eos_token_id=None)      # p == 1: a state without the penalty's operands
    st1 = next(reversed(dec.graphs.values()))
    assert "pen" not in st1 and "pen_out" not in st1 and "pen_t" not in st1
    assert c.tolist() == _hf(model, dev, eos_token_id=None).tolist()


def test_the_kernel_runs_in_the_step(dev):
    """Eager steps under the profiler: p != 1 launches repetition_penalty_kernel, p == 1 and the statement form do not."""
    x, m = GL._inputs(dev, torch.bfloat16, 3)
    kw = dict(attention_mask=m, pad_token_id=0, use_graph=False)
    dec = _decoder("llama", dev, torch.bfloat16)
    _, names = GL._kernel_names(lambda: dec.generate(x, 4, repetition_penalty=P_, **kw))
    assert any("repetition_penalty_kernel" in k for k in names), names
    _, names = GL._kernel_names(lambda: dec.generate(x, 4, **kw))
    assert not any("repetition_penalty_kernel" in k for k in names)
    _, names = GL._kernel_names(lambda: _decoder("llama", dev, torch.bfloat16, False).generate(x, 4, repetition_penalty=P_, **kw))
    assert not any("repetition_penalty_kernel" in k for k in names)


@pytest.mark.parametrize("model", MODELS)
def test_graph_generate_with_and_without_the_opt_in(dev, model):
    from videotgb_amd import decode as D
    M = _mod(model)
    lm = _lm(model, dev, torch.float32)
    x, m = M._inputs(dev, torch.float32, 3)
    cfgs = dict(do_sample=False, max_new_tokens=M.N_NEW, num_beams=1, repetition_penalty=P_, eos_token_id=None, pad_token_id=0)
    owner = types.SimpleNamespace(penalty_decode="graph")
    out = D.graph_generate(owner, lm, x, m, cfgs)
    assert out is not None and owner._decoder.penalty is True and owner._decoder.fused
    assert _gen(model, out).tolist() == _hf(model, dev, repetition_penalty=P_, eos_token_id=None).tolist()
    assert "pen_out" in next(reversed(owner._decoder.graphs.values()))
    assert D.graph_generate(types.SimpleNamespace(), lm, x, m, cfgs) is None
    assert D.graph_generate(types.SimpleNamespace(penalty_decode="hf"), lm, x, m, cfgs) is None
