"""CPU-side checks of the clip-session API: the factory exists on both model flavours and the host-side validation rejects inputs that are
not one clip before any device work starts."""
import pytest
import torch


def test_factory_on_both_flavours():
    from videotgb_amd import models
    from videotgb_amd.session import ClipSession
    for cls in (models.LSTP, models.LSTP_blip2):
        assert callable(getattr(cls, "clip_session"))
    assert callable(ClipSession.generate) and callable(ClipSession.prefetch)
    for name in ("trunk", "resume"):
        assert callable(getattr(models.TemporalEncoder, name))


@pytest.mark.parametrize("frames,flow,of", [
    ((2, 8, 3, 56, 56), (1, 12, 3, 224, 224), None),      # two clips of candidates
    ((8, 3, 56, 56), (2, 12, 3, 224, 224), None),         # two clips of flow frames
    ((8, 3, 56, 56), None, (2, 12, 2, 224, 224)),         # two clips of flow
    ((8, 3, 56, 56), None, None),                         # no flow at all
    ((3, 56, 56), (1, 12, 3, 224, 224), None),            # not a frame stack
])
def test_constructor_rejects_more_than_one_clip(frames, flow, of):
    from videotgb_amd.session import ClipSession
    mk = (lambda s: None if s is None else torch.zeros(s))
    with pytest.raises(ValueError):
        ClipSession(object(), mk(frames), mk(flow), mk(of))     # (validation runs before the model is touched)


def test_tgb_trunk_object():
    from videotgb_amd import ops
    t = ops.TgbTrunk(torch.zeros(98, 8), torch.zeros(98, 8), torch.ones(1, 98, dtype=torch.long), "fusion", ops.F32)
    assert t.L == 96 and t.mode == "fusion"
    with pytest.raises(ValueError, match="INVALID MODE"):
        ops.tgb_trunk(None, torch.zeros(1, 4, 2, 224, 224), torch.ones(1, 6, dtype=torch.long), "bogus")
