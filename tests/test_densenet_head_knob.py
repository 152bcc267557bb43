import pytest

from triton_client_amd.server.gpu_models import DensenetOnnx


@pytest.mark.parametrize("value,want", [(None, "lib"), ("0", "lib"), ("1", "fused"), ("2", "lib"), ("", "lib")])
def test_the_knob_selects_the_classifier(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("TCAMD_DENSENET_HEAD", raising=False)
    else:
        monkeypatch.setenv("TCAMD_DENSENET_HEAD", value)
    assert DensenetOnnx.head_classifier() == want
