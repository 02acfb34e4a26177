"""Variable-length batches of the speech-length predictor: everything that is decided on the host.  Lengths are validated
(varlen.validate_lengths) before any device is touched, so a bad length is a ValueError on a GPU-less machine too and the
"no CPU path" error comes only after it; SpeechGenerator.predict_frames is class -> seconds -> frames arithmetic."""
import pytest
import torch

from ditto_tts_amd.modules import DiTTO
from ditto_tts_amd.sampler import SpeechGenerator
from ditto_tts_amd.shipped_config import ConfigSLP
from ditto_tts_amd.slp import SLP

B, S, T, D = 3, 12, 8, 64


@pytest.fixture(scope="module")
def slp():
    return SLP(5, 1, 1, hidden_size=D).eval()


@pytest.fixture(scope="module")
def z():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, T, D, generator=g), torch.randn(B, S, D, generator=g)


@pytest.mark.parametrize("kw", [
    {"audio_lengths": [3, 4]},                                  # wrong count
    {"text_lengths": [1, 2, 3, 4]},
    {"audio_lengths": [3, 0, 5]},                               # a value of 0
    {"text_lengths": (0, 1, 1)},
    {"audio_lengths": [3, S + 1, 5]},                           # above S
    {"text_lengths": [T + 1, 1, 1]},                            # above T
    {"audio_lengths": torch.tensor([3.0, 4.0, 5.0])},           # a float tensor
    {"text_lengths": torch.tensor([True, True, True])},         # a bool tensor
    {"audio_lengths": [3, 4, 5], "text_lengths": [1, 2, T + 1]},   # a good one does not excuse a bad one
    {"audio_lengths": torch.tensor([[3, 4, 5]])},               # wrong shape
    {"audio_lengths": [3, True, 5]},                            # a bool in a list
    {"text_lengths": 4},                                        # not a sequence
])
def test_bad_lengths_raise_before_any_device_use(slp, z, kw):
    z_text, z_audio = z
    with pytest.raises(ValueError):
        slp.decode(z_text, z_audio, **kw)          # CPU tensors: a device check first would raise RuntimeError instead
    with pytest.raises(ValueError):
        slp.predict_class(z_text, z_audio, **kw)


@pytest.mark.parametrize("kw", [
    {"audio_lengths": [3, 4, S]}, {"text_lengths": torch.tensor([1, T, 2])},
    {"audio_lengths": (1, 1, 1), "text_lengths": torch.tensor([T, T, T], dtype=torch.int32)}, {},
])
def test_cpu_tensors_are_refused_only_after_validation(slp, z, kw):
    z_text, z_audio = z
    with pytest.raises(RuntimeError, match="no CPU path"):
        slp.decode(z_text, z_audio, **kw)
    with pytest.raises(ValueError):                # shape errors come first as well
        slp.decode(z_text[:2], z_audio, audio_lengths=[1, 1, 1])


class StubSLP:
    """Stands in for SLP: fixed classes, and a record of what it was asked."""

    def __init__(self, classes):
        self.classes, self.calls = torch.tensor(classes, dtype=torch.int64), []

    def predict_class(self, z_text, z_audio, *, audio_lengths=None, text_lengths=None):
        self.calls.append((audio_lengths, text_lengths))
        return self.classes


@pytest.fixture(scope="module")
def ditto_model():
    return DiTTO(128, 1, 2, 64, 128, 6)


def test_predict_frames_arithmetic(ditto_model, z):
    z_text, z_audio = z
    stub = StubSLP([0, 4, 10])
    sg = SpeechGenerator(ditto_model=ditto_model, device="cpu", slp=stub)
    t0 = ConfigSLP.MIN_AUDIO_DURATION
    assert t0 == 10                                # the reference's label is int(duration - 10), src/utils/MLS.py:77
    got = sg.predict_frames(z_text, z_audio, frame_rate=75, audio_lengths=[3, 4, 5], text_lengths=[1, 2, 3])
    assert got == [750, 1050, 1500] and all(type(v) is int for v in got)
    assert stub.calls[-1] == ([3, 4, 5], [1, 2, 3])                      # the lengths reach the predictor
    assert sg.predict_frames(z_text, z_audio, frame_rate=21.5) == [215, 301, 430]
    assert stub.calls[-1] == (None, None)
    assert sg.predict_frames(z_text, z_audio, frame_rate=0.26) == [round(10 * 0.26), round(14 * 0.26), round(20 * 0.26)]
    # a caller's own class -> seconds map
    got = sg.predict_frames(z_text, z_audio, frame_rate=50, seconds_of_class=lambda c: 0.5 * c + 0.25)
    assert got == [round(0.25 * 50), round(2.25 * 50), round(5.25 * 50)]


def test_frame_rate_is_required_and_slp_is_needed(ditto_model, z):
    z_text, z_audio = z
    sg = SpeechGenerator(ditto_model=ditto_model, device="cpu", slp=StubSLP([1, 2, 3]))
    with pytest.raises(TypeError):
        sg.predict_frames(z_text, z_audio)
    with pytest.raises(TypeError):
        sg.predict_frames(z_text, z_audio, 75)     # keyword only: no positional guess either
    for bad in (0, -75, None, "75", True):
        with pytest.raises(ValueError, match="frame_rate"):
            sg.predict_frames(z_text, z_audio, frame_rate=bad)
    bare = SpeechGenerator(ditto_model=ditto_model, device="cpu")
    with pytest.raises(RuntimeError, match="slp is not available"):
        bare.predict_frames(z_text, z_audio, frame_rate=75)
