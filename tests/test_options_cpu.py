"""CPU test of the csm_set_option switchboard: every key is known to the library and asks for an engine
(no GPU is touched: a null engine is rejected before any device call)."""
from csm_mlx import _lib

OPTION_KEYS = (
    "linear_mfma", "fold_proj", "qkv0_tab", "dec_frame", "bb_step", "gemm_xs", "bb_xs", "qkv0_tab_batched",
    "attn_prefill",
    "dec_frame_stamps", "bb_step_stamps", "dec_xsd_stamps", "dec_xsd", "dec_xsd_head", "dec_xsd_sample",
    "prefill_rows", "inject_handoff_error",
)


def test_every_option_key_needs_an_engine():
    L = _lib.lib()
    for key in OPTION_KEYS:
        for value in (0, 1):
            assert L.csm_set_option(None, key.encode(), value) == _lib.CSM_ERR_ARG, key
            msg = L.csm_last_error().decode()
            assert msg.startswith(key + " needs an engine"), (key, msg)


def test_unknown_option_key():
    L = _lib.lib()
    for key in (b"no_such_option", b"", b"dec_frame_", b"stamps"):
        assert L.csm_set_option(None, key, 1) == _lib.CSM_ERR_ARG, key
        assert "unknown option" in L.csm_last_error().decode(), key
