"""CPU: the output_attentions surface exists at every level of the model and the kernel behind it is part of the C-ABI."""
import inspect


def test_forward_accepts_output_attentions_at_each_level(built_lib):
    from vacnic_amd.models import mmbart as M
    for cls in (M.BartAttention, M.BartEncoderLayer, M.BartDecoderLayer, M.BartEncoder, M.BartDecoder, M.BartModel,
                M.BartForMultiModalGeneration):
        params = inspect.signature(cls.forward).parameters
        assert "output_attentions" in params, f"{cls.__name__}.forward has no output_attentions"
        assert params["output_attentions"].default in (None, False), f"{cls.__name__}: output_attentions must default to off"


def test_config_has_output_attentions_off_by_default():
    from vacnic_amd.config import VacnicConfig
    assert VacnicConfig().output_attentions is False


def test_attn_probs_is_exported_and_bound(built_lib):
    import ctypes
    from vacnic_amd import _lib, kernels
    assert "vacnic_attn_probs" in _lib.EXPORTED
    assert hasattr(ctypes.CDLL(built_lib), "vacnic_attn_probs")
    assert _lib._STRUCT_FNS["vacnic_attn_probs"].__name__ == "vacnic_attn_probs_args"
    sig = inspect.signature(kernels.attn_probs)
    assert list(sig.parameters) == ["q", "k", "B", "H", "Tq", "Tk", "key_mask", "causal", "scale"]
    assert sig.parameters["scale"].default == 0.125 and sig.parameters["causal"].default is False
