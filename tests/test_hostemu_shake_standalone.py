"""tests/shake_standalone.py on the host-emulated kernels: every standalone shake family meets its float64 reference bounds with its
guard bands intact and is the same run to run, before tests/test_gpu_shake_standalone.py spends GPU time on it.  (Emulated workgroups
run their threads in step: a missing barrier cannot show here, which is what the GPU module is for.)"""
import pytest

from audiblelight_amd import _hip, engine
from tests import hostemu, shake_standalone as ss


@pytest.fixture(scope="module")
def emu():
    return engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())


@pytest.mark.parametrize("family", list(ss.FAMILIES))
def test_emu_standalone_family(emu, family):
    first = ss.FAMILIES[family](emu)
    assert first and set(first) == set(first.eps)
    again = ss.FAMILIES[family](emu)
    assert ss.same(first, again) and ss.worst_ratio(first, again) == 0.0
