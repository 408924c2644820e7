"""tests/fx_batch_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_fx_batch.py with the workgroups
of a batch running side by side, plus scenario 1 once on the AL_SHAKE=3 build of tests/shake.py (`s3w`: wave 0 of every workgroup
the last to leave each barrier), whose batched outputs must be the product library's, bit for bit."""
import numpy as np
import pytest

from tests import fx_batch_cases as cases
from tests import kernel_edges as ke

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.fixture(scope="module")
def batched(gpu):
    """kind -> the outputs of scenario 1 on the product library (each kind's batch runs once here)"""
    return {}


@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_batch_equals_single_clip_launches(gpu, batched, kind):
    batched[kind] = cases.run_batch_equals_singles(gpu, kind)


@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_batch_of_one(gpu, kind):
    cases.run_batch_of_one(gpu, kind)


def test_sos_batch_in_place(gpu):
    cases.run_batch_equals_singles(gpu, "sos", in_place=True)


def test_refusals_name_the_job(gpu):
    cases.run_refusals(gpu)


def test_run_chains_equal_the_per_event_loop(gpu, monkeypatch):
    cases.run_chains_equal_the_loop(gpu, monkeypatch)


def test_scene_equals_the_per_event_loop(gpu, monkeypatch):
    cases.run_scene_equals_the_loop(gpu, monkeypatch)


def test_shaken_batches_render_the_product_bits(gpu, batched):
    from audiblelight_amd import _hip, engine
    from tests import shake

    shaken = engine.Renderer(lib=_hip.Library(shake.existing_or_built(["s3w"])["s3w"]))
    for kind in cases.KINDS:
        want = batched[kind] if kind in batched else cases.run_batch(gpu, kind, cases.specs(kind))
        got = cases.run_batch_equals_singles(shaken, kind)      # on the shaken build too: its own single-clip launches, the bounds, the guards
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(ke.bits(g), ke.bits(w)), (kind, i)
