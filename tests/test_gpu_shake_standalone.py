"""The barrier kernels outside the render stage, shaken (tests/shake_standalone.py; the render stage: tests/test_gpu_shake.py).

Neither the host emulation (no concurrent waves) nor the product build (whose waves usually arrive in a lucky order) can see a
missing or misplaced workgroup barrier in the FX scans, the block reductions or the encode transpose.  Here every standalone family
runs through the product library and through the schedule-perturbed builds of tests/shake.py.  On each library every launch must
meet its float64 reference bound with its guard bands intact (the scenario runners assert that); then the outputs must be

  - bit-identical run to run on the product library and on `s1`,
  - bit-identical between `s1` and `s3w` (different skews),
  - within the sum of the two reference bounds of the product library's (both met their bound against the same reference, so this
    follows by the triangle inequality: no tolerance of this module's own), and EQUAL to them for the families in
    BIT_IDENTICAL_TO_PRODUCT.

The `revert` variant compiles out one barrier of k_fx_sos and one of k_fx_delay (csrc/al_sos.h, csrc/al_delayfx.h): the tests at the
end must catch both, or the module proves nothing for those kernels.  The words left unsynchronised there are sample and state
values only -- never an index, a pointer or a loop bound -- and every thread still executes the same number of barriers, so such a
build renders wrong samples and cannot fault or hang.

Measured: profiles/r08_shake_standalone.txt.
"""
import time

import pytest

from tests import shake, shake_standalone as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def product():
    from audiblelight_amd import engine

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    return r


@pytest.fixture(scope="module")
def shaken():
    from audiblelight_amd import _hip, engine

    paths = shake.existing_or_built(["s1", "s3w"])
    return {name: engine.Renderer(lib=_hip.Library(path)) for name, path in paths.items()}


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[shake standalone] module wall time {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("family", list(ss.FAMILIES))
def test_every_standalone_family_is_schedule_independent(product, shaken, family):
    run = ss.FAMILIES[family]
    ref = run(product)
    assert ss.same(ref, run(product)), "the product library is not deterministic run to run"
    s1, s3w = run(shaken["s1"]), run(shaken["s3w"])
    assert ss.same(s1, s3w), (family, [k for k in s1 if not ss.same({k: s1[k]}, {k: s3w[k]})])
    assert ss.same(s1, run(shaken["s1"])), "a schedule-perturbed build is not deterministic run to run"
    ratio, identical = ss.worst_ratio(s1, ref), ss.same(s1, ref)
    print(f"\n[shake standalone] {family}: bit-identical to product {'yes' if identical else 'no'}, "
          f"worst |shaken - product| / (sum of the two reference bounds) {ratio:.3g}")
    assert ratio <= 1.0, (family, ratio)
    if family in ss.BIT_IDENTICAL_TO_PRODUCT:
        assert identical, (family, [k for k in s1 if not ss.same({k: s1[k]}, {k: ref[k]})])


@pytest.mark.parametrize("family", ["fx_sos", "fx_delay"])
def test_a_dropped_barrier_is_caught(shaken, family):
    """tests/shake.py's `revert` variant = the shaken sources WITHOUT the barrier between filtering and write-back in sos_sweep
    (AL_TEST_REVERT_SOS_BARRIER: the copy-out reads LDS rows their owners have not filtered yet) and WITHOUT the second barrier of
    k_fx_delay's scan loop (AL_TEST_REVERT_DELAY_BARRIER: a wave's next carry[tid] = w overtakes another wave's read of the old
    one).  At most four runs of the family; a mismatch against `s1` counts, and so does a missed reference bound (the runners'
    AssertionError).  Nothing differing fails: no longer loop to force it."""
    from audiblelight_amd import _hip, engine

    r = engine.Renderer(lib=_hip.Library(shake.existing_or_built(["revert"])["revert"]))
    ref = ss.FAMILIES[family](shaken["s1"])
    caught_at = None
    for attempt in range(1, 5):
        try:
            differs = not ss.same(ref, ss.FAMILIES[family](r))
        except AssertionError:
            differs = True
        if differs:
            caught_at = attempt
            break
    print(f"\n[shake standalone] revert in {family}: caught at run {caught_at}")
    assert caught_at is not None, f"the build without a barrier of {family} renders the same bits: this module would not have caught it"
