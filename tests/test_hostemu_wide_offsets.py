"""tests/wide_offset_cases.py on the host-emulated kernels: sections A (render stage), B (mixdown) and C (image-source rows).  The
host build compiles the same index expressions as the gfx950 build, so a 32-bit overflow in them shows here as well.  The memory
provider of this file allocates UNTOUCHED (np.empty): a buffer of 16 GiB costs address space, and only the pages a case writes
cost memory.  Where the host cannot reserve that address space the case skips and says so."""
import gc

import numpy as np
import pytest

from audiblelight_amd import _hip, engine
from tests import hostemu, wide_offset_cases as wo


class UntouchedMemory(hostemu.NumpyMemory):
    def empty(self, n, dtype=np.float32):
        try:
            return np.empty(max(int(n), 1), dtype=dtype)
        except MemoryError:
            pytest.skip(f"this host cannot reserve {max(int(n), 1) * np.dtype(dtype).itemsize} bytes of address space")


@pytest.fixture(scope="module")
def emu():
    return engine.Renderer(lib=_hip.Library(hostemu.build()), memory=UntouchedMemory())


@pytest.fixture(autouse=True)
def release():
    yield
    gc.collect()


@pytest.fixture(scope="module", autouse=True)
def margins():
    wo.rd.MARGINS.clear()
    yield
    for family, (seen, bound) in sorted(wo.rd.MARGINS.items()):
        print(f"\n[host emulation] {family}: worst {seen:.3g}, bound {bound:.3g}")


LAYOUTS = [(10, "plain"), (13, "split"), (14, "quad")]


def partitions(log2_block):
    return 1 if log2_block == 14 else 2        # one partition at B = 16384: the emulated transforms of a second one cost seconds


@pytest.mark.parametrize("position", ["i31", "i32", "b32"])
@pytest.mark.parametrize("log2_block,layout", LAYOUTS)
def test_emu_spatial(emu, log2_block, layout, position):
    wo.run_spatial(emu, log2_block, layout, position, P=partitions(log2_block))


@pytest.mark.parametrize("position", ["i31", "i32", "b32"])
@pytest.mark.parametrize("log2_block,layout", LAYOUTS)
def test_emu_audio(emu, log2_block, layout, position):
    wo.run_audio(emu, log2_block, layout, position, P=partitions(log2_block))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("which", ["n", "c"])
@pytest.mark.parametrize("log2_block,layout", LAYOUTS)
def test_emu_ir_strides(emu, log2_block, layout, which, fused):
    wo.run_ir_strides(emu, log2_block, layout, which, fused, P=partitions(log2_block))


@pytest.mark.parametrize("position", ["i31", "b32"])
@pytest.mark.parametrize("log2_block,layout", LAYOUTS)
def test_emu_spectra_bases(emu, log2_block, layout, position):
    wo.run_spectra_bases(emu, log2_block, layout, position, P=partitions(log2_block))


@pytest.mark.parametrize("name", [c[0] for c in wo.MAC_CASES])
def test_emu_mac_regime(emu, name):
    wo.run_mac_regime(emu, name)


def test_emu_python_layer(emu):
    wo.run_python_layer(emu)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("position", ["i31", "i32", "b32"])
def test_emu_mix_slot_src(emu, position, accumulate):
    wo.run_mix_slot_src(emu, position, accumulate=accumulate)


# The two cases below are real passes over 2^31 floats -- k_mixdown writes every sample of the scene, the image-source kernels every
# pad sample of every row, whatever the test looks at -- which the emulation makes in about two minutes each.  One case each:
# the only net on the build host under the row bases of k_mixdown and k_ism_shoebox; the others run on the gfx950 build.
def test_emu_mix_row_base(emu):
    wo.run_mix_row_base(emu, 2_880_001, accumulate=False, ambience=True)


def test_emu_ism_shoebox(emu):
    wo.run_ism_shoebox(emu, tail=True)


def test_emu_dry_fetch(emu):
    wo.run_dry_fetch(emu)
