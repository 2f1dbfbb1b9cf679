"""The error contract of the fused pass, as far as it shows without a device: the host extension has ONE exception type for "this
chunk is outside the pass" and it is nmf_amd.fast_step.Unsupported; every other failure of the C++ pass keeps its own type, so that no
caller mistakes it for a chunk to re-run through the operator graph."""
import pytest
import torch

from nmf_amd import fast_step, hip


def test_only_a_chunk_outside_the_pass_is_unsupported():
    assert hip.HOST_EXT.unsupported_class() is fast_step.Unsupported
    assert not issubclass(fast_step.Unsupported, RuntimeError) and not issubclass(hip.NmfHipError, fast_step.Unsupported)
    core = hip.HOST_EXT.StepCore()                  # (constructed without a device)
    assert not core.has_pending()
    with pytest.raises(RuntimeError, match="without a pending train_forward") as e:
        core.train_backward(torch.zeros(1, 3), None, None, True)
    assert not isinstance(e.value, fast_step.Unsupported)
