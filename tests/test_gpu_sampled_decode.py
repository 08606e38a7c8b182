"""-m gpu: a LightningModule twin with the shipped SAMPLED ``generate_configs`` (LSTP_instructblip.yaml: do_sample, top_p 0.9,
max_length 250, min_length 1) on a tiny fp32 Llama, ``temperature`` set to 1e-6 so that the warped distribution collapses onto the greedy
token and the ids can be compared with HF.  Built with sampled_decode="graph", ``eval_forward`` goes through ``decode.graph_generate`` and
the Llama graph decoder's sampling path: a tensor of at most ``max_length - P`` columns whose ids equal HF greedy ``generate``'s, twice over
the same cached sampled state.  The same twin without the opt-in gets None from the planner and runs HF generate, as before."""
import pytest
import torch

import test_gpu_beam_decode as GB      # the tiny instructblip twin

pytestmark = pytest.mark.gpu

LSTP_INSTRUCTBLIP_YAML = dict(length_penalty=1, repetition_penalty=1.0, num_beams=1, min_length=1, max_length=250, top_p=0.9, temperature=1.0, do_sample=True)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def test_a_llama_twin_with_the_shipped_sampled_generate_configs(dev, tmp_path, monkeypatch):
    from videotgb_amd import decode
    m, batch, noise = GB._sf_module(dev, tmp_path, sampled_decode="graph")
    assert m.sampled_decode == "graph"
    real, seen = decode.graph_generate, []

    def spy(owner, lm, inputs_embeds, attention_mask, generate_configs):
        out = real(owner, lm, inputs_embeds, attention_mask, generate_configs)
        seen.append((out, inputs_embeds.shape[1]))
        return out
    monkeypatch.setattr(decode, "graph_generate", spy)
    cold = dict(LSTP_INSTRUCTBLIP_YAML, temperature=1e-6)      # the literal dict, its distribution collapsed onto the greedy token

    m.sampled_decode = "hf"      # without the opt-in: the planner answers None and HF generate runs, greedy and sampled
    m.generate_configs = dict(cold, do_sample=False)
    greedy = m.eval_forward(batch, noise=noise)
    m.generate_configs = dict(cold)
    hf_cold = m.eval_forward(batch, noise=noise)
    assert [s[0] for s in seen] == [None, None] and getattr(m, "_decoder", None) is None
    P = seen[0][1]
    assert 1 < greedy.shape[1] <= 250 - P and hf_cold.tolist() == greedy.tolist()

    m.sampled_decode = "graph"
    first = m.eval_forward(batch, noise=noise)
    out = seen[-1][0]
    assert isinstance(out, torch.Tensor) and out.shape[0] == greedy.shape[0] and out.shape[1] <= 250 - P
    assert first.tolist() == greedy.tolist()
    dec = m._decoder
    st = next(reversed(dec.graphs.values()))
    assert st["out"].shape[1] == 250 - P and st["sample"] is not None and st["sample"][0] == 1e-6 and st["sample"][2] == 0.9 and st["min_new"] == 0
    assert st["graph"] is not None      # (the steps were replayed)
    again = m.eval_forward(batch, noise=noise)      # the cached sampled state and its captured graph, a second time
    assert m._decoder is dec and len(dec.graphs) == 1 and next(reversed(dec.graphs.values())) is st
    assert isinstance(seen[-1][0], torch.Tensor) and again.tolist() == greedy.tolist()
