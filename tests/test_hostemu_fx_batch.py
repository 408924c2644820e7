"""Batched FX launches (tests/fx_batch_cases.py) on the host-emulated kernels: per kind a batch against the same jobs through the
single-clip entry, bit for bit and against the float64 bound of the kind's own case module; a batch of one; SOS in place; the
refusals of al_fx_batch_pack with their job index; augmentation.run_chains against the per-event loop with the launches counted;
a scene through core.stage_event_chains.  The gfx950 build runs the same scenarios in tests/test_gpu_fx_batch.py, where the
workgroups of a batch do run concurrently."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import fx_batch_cases as cases
from tests import hostemu


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_emu_batch_equals_single_clip_launches(emu, kind):
    cases.run_batch_equals_singles(emu, kind)


@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_emu_batch_of_one(emu, kind):
    cases.run_batch_of_one(emu, kind)


def test_emu_sos_batch_in_place(emu):
    cases.run_batch_equals_singles(emu, "sos", in_place=True)


def test_emu_refusals_name_the_job(emu):
    cases.run_refusals(emu)


def test_emu_run_chains_equal_the_per_event_loop(emu, monkeypatch):
    cases.run_chains_equal_the_loop(emu, monkeypatch)


def test_emu_scene_equals_the_per_event_loop(emu, monkeypatch):
    cases.run_scene_equals_the_loop(emu, monkeypatch)
