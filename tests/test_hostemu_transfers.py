"""The render-stage scenarios of tests/transfer_cases.py on the host-emulated kernels: the gaps of the packed audio, AL_TRIM_PARTITIONS=0
and AL_STATIC_MAC_MAX_P need no device memory provider, so their index arithmetic is checked on CPU too.  The transfer paths
themselves (TorchMemory, BatchDriver) only exist on the GPU: tests/test_gpu_transfers.py."""
import pytest

from audiblelight_amd import _hip, engine
from tests import hostemu, transfer_cases as tc
from tests.conftest import set_switch


@pytest.fixture(scope="module")
def emu():
    return engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())


@pytest.mark.parametrize("fold", [False, True], ids=["plain_clips", "folded_clips"])
@pytest.mark.parametrize("layout,log2_block", tc.GAP_LAYOUTS, ids=[f"{name}{lb}" for name, lb in tc.GAP_LAYOUTS])
def test_emu_audio_gaps_are_never_read(emu, layout, log2_block, fold):
    tc.run_gap_render(emu, log2_block, layout, fold)


def test_emu_trim_partitions_off(emu, monkeypatch):
    tc.run_untrimmed_moving(emu, lambda name, value: set_switch(monkeypatch, name, value))


def test_emu_static_mac_max_p(emu, monkeypatch):
    tc.run_static_mac_max_p(emu, lambda name, value: set_switch(monkeypatch, name, value), 11)
