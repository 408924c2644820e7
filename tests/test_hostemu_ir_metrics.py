"""The room-acoustic metrics of an IR tensor (tests/ir_metrics_cases.py) on the host-emulated kernels: all 16 columns and the knots
of every row against the float64 restatement within the derived bound, at every row length at which the code takes another path
(1, 2, around a knot, around the workgroup tile, nine tiles), at the tight and a larger pitch, a larger stride_c with a sentinel
between the rows, the odd pitch at an unaligned base (the scalar arm), without knots; the peak at the first and the last sample, in
the last tile and on a tile boundary, equal maxima, thresholds crossed in a later tile, a decay that reaches -25 but not -35 dB, rows
too short for a fit, windows past the end, silent and non-finite rows; the identity of a row alone and among others; the second
capsule's rows past element 2^31; the refusals of the C ABI and of the Python layer; the states and the JSON round trip.  The gfx950
build runs the same scenarios in tests/test_gpu_ir_metrics.py."""
import gc

import numpy as np
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import ir_metrics_cases as cases
from tests.wide_offset_cases import need, reserve


class UntouchedMemory(hostemu.NumpyMemory):
    """np.empty: a buffer of 8 GiB costs address space, and only the pages a case writes cost memory."""

    def empty(self, n, dtype=np.float32):
        try:
            return np.empty(max(int(n), 1), dtype=dtype)
        except MemoryError:
            pytest.skip(f"this host cannot reserve {max(int(n), 1) * np.dtype(dtype).itemsize} bytes of address space")


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)
    for name, frac in sorted(cases.WORST.items()):
        print(f"\n[host emulation] ir metrics, {name}: worst error / bound {frac:.3g}")


@pytest.mark.parametrize("ir_len", cases.LENGTHS)
def test_emu_parity_and_layouts(emu, ir_len):
    cases.run_length(emu, ir_len)


def test_emu_nine_tiles(emu):
    cases.run_tiled(emu)


def test_emu_short_row_features(emu):
    cases.run_features(emu)


def test_emu_silent_and_non_finite_rows(emu):
    cases.run_special(emu)


def test_emu_identity(emu):
    cases.run_identity(emu)


def test_emu_second_capsule_past_element_2_31():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=UntouchedMemory())
    cases.run_wide(r, "i31", reserve, need)
    gc.collect()


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu):
    cases.run_python_errors(emu)


def test_emu_state_and_host_arrays(emu):
    cases.run_state(emu)


def test_emu_dictionary_round_trip(emu):
    cases.run_round_trip(emu)
