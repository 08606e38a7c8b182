"""CPU: the drop-in registration (videotgb_amd/dropin.py).  The first test checks what ``install()`` registers; the second loads a
reference-layout Lightning checkpoint the way the reference's eval loader does (``eval/utils/builder_utils.load_pretrained_model``,
twinned by videotgb_amd.builder_utils) and checks that it ends up constructing and loading the HIP-backed ``LSTP`` that the drop-in
hands to that loader under ``eval.utils.model``."""
import importlib
import sys

import torch

from conftest import full_state_dict, write_hf_config


def test_install_registers_the_reference_module_paths():
    from videotgb_amd import dropin, models, modules
    names = dropin.install()
    try:
        assert "eval.utils.model" in names and len(names) == 1 + len({t.rsplit(".", 1)[0] for t in modules.TARGETS})
        for target, cls in modules.TARGETS.items():      # what hydra.utils.instantiate(_target_=...) does: import module, getattr
            mod, attr = target.rsplit(".", 1)
            assert getattr(importlib.import_module(mod), attr) is cls
        from eval.utils.model import LSTP, LSTP_blip2     # noqa: the statement eval/utils/builder_utils.py:14 executes
        assert LSTP is models.LSTP and LSTP_blip2 is models.LSTP_blip2
    finally:
        dropin.uninstall()
    assert "eval.utils.model" not in sys.modules and "src.models.LSTP_module" not in sys.modules
    # constructor signatures are the reference's (eval/utils/model.py:21-26; src/models/LSTP_module.py:85-95)
    import inspect
    assert list(inspect.signature(models.LSTP.__init__).parameters)[1:4] == ["base_model_path", "device", "lora"]
    assert list(inspect.signature(modules.LSTPModule.__init__).parameters)[1:9] == [
        "model_name_or_path", "sampler_name_or_path", "of_extractor_name_or_path", "temperature", "optimizer", "scheduler",
        "scheduler_params", "generate_configs"]


def test_loader_builds_the_dropin_hip_model_from_a_reference_checkpoint(tmp_path):
    from videotgb_amd import builder_utils, dropin, models, synth
    from videotgb_amd.synth import tiny_cfg
    dropin.install()
    try:
        from eval.utils.model import LSTP     # noqa: the class eval/utils/builder_utils.py:14 imports
        cfg = tiny_cfg("instructblip")
        cfg.vit.image = 56
        base = write_hf_config(str(tmp_path / "instructblip-tiny"), "instructblip", cfg)
        # the reference's constructor call has no way to shrink the TGB: it is BERT-base (BertConfig(fusion_layer=6,
        # encoder_width=768)), so the checkpoint carries a full-size temporal_encoder
        cfg.tgb = synth.TgbCfg()
        sd = full_state_dict(cfg, models.build_language_model(models.load_hf_config(base, "instructblip")))
        ckpt = str(tmp_path / "last.ckpt")
        torch.save({"state_dict": sd}, ckpt)
        # the reference loader's positional call (ckpt, base, sampler path, device, lora); strict load of ckpt["state_dict"]
        model, proc, sproc = builder_utils.load_pretrained_model(ckpt, base, "bert-base-uncased", "cpu", False, load_processors=False)
        assert type(model) is LSTP and (proc, sproc) == (None, None)
        got = model.state_dict()
        for k in ("model.qformer.encoder.layer.0.attention.attention.query.weight", "temporal_encoder.mrc_head.weight",
                  "of_extractor.update_block.gru.convz1.weight", "model.language_model.lm_head.weight"):
            assert torch.equal(got[k], sd[k].to(got[k].dtype)), k       # (the LLM is built in bf16 with the default compute dtype)
        assert hasattr(model, "generate") and model.model.config.use_decoder_only_language_model
    finally:
        dropin.uninstall()
