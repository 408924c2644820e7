"""The device shoebox IR generator (tests/shoebox_cases.py) on the host-emulated kernel: the anechoic room, parity with the float64
oracle of the definition within the derived bound (two rooms, six unequal walls, four order limits, 1x1 and 3x5 pairs, two sample
rates), row lengths around the tap count and the tile into guarded buffers, a capsule 1 cm from its source, a tile with more images
than a chunk or a list holds, bit-level determinism, the refusals of the C ABI and of the Python layer, Sabine's law both ways, the
state and its lazy tensor, a scene end to end without the tensor touching the host.  The gfx950 build runs the same scenarios in
tests/test_gpu_shoebox.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import shoebox_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


def test_emu_anechoic_room_is_one_image(emu):
    cases.run_anechoic(emu)


@pytest.mark.parametrize("room,order,pairs,fs", cases.PARITY)
def test_emu_parity_with_oracle(emu, room, order, pairs, fs):
    cases.run_parity(emu, room, order, pairs, fs)


@pytest.mark.parametrize("ir_len", cases.EDGE_LEN)
def test_emu_edge_lengths(emu, ir_len):
    cases.run_edge_length(emu, ir_len)


def test_emu_capsule_one_centimetre_from_source(emu):
    cases.run_close_capsule(emu)


def test_emu_more_images_than_a_chunk_or_a_list(emu):
    cases.run_crowded_tile(emu)


def test_emu_determinism(emu):
    cases.run_determinism(emu)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu):
    cases.run_python_errors(emu)


def test_emu_rt60_round_trip():
    cases.run_rt60_round_trip()


def test_emu_state_and_lazy_tensor(emu):
    cases.run_state_and_tensor(emu)


def test_emu_scene_end_to_end(emu, monkeypatch, tmp_path):
    cases.run_end_to_end(emu, monkeypatch, tmp_path)
