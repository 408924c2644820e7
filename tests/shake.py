"""Schedule-perturbed builds of the HIP library (TEST INFRASTRUCTURE, never loaded by the package).

``-DAL_SHAKE=<seed>`` (audiblelight_amd/csrc/al_common.h) makes every wave sleep a wave-, workgroup- and site-dependent number of cycles
around every workgroup barrier, after every LDS-DMA issue and before every hand-counted ``s_waitcnt``: the inline-asm paths that
the host-emulation build -- and with it ASan / UBSan and the differential fuzz -- cannot see.  tests/test_gpu_shake.py renders one
batch per kernel family through each variant, tests/test_gpu_shake_standalone.py launches the barrier kernels outside the render
stage (tests/shake_standalone.py: FX scans, statistics, encode) from each; both assert bit-identical output between the perturbed
builds and run to run, and a derived bound against the product library.

Variants (built in-tree under tests/shake_build/ by ``__graft_entry__.build()`` so that they travel to the GPU box like the product
.so; about as long to compile as the product library, all of them side by side):
  s1      AL_SHAKE=1: pseudo-random skews
  s3w     AL_SHAKE=3 (wave 0 always last to move on) + AL_Q16_WAVES=1 + AL_SPLIT_WAVES=2 (other register budgets / occupancies)
  revert  AL_SHAKE=3 + three barriers compiled out, each in a kernel the others' families never launch -- the variant the tests
          must FAIL on:
            AL_TEST_REVERT_Q16_BARRIER    the round-4 LDS race of al_quad16.h re-introduced (test_gpu_shake.py)
            AL_TEST_REVERT_SOS_BARRIER    sos_sweep (al_sos.h) without the barrier between filtering a tile and writing it back
            AL_TEST_REVERT_DELAY_BARRIER  k_fx_delay (al_delayfx.h) without the second barrier of its scan loop
          (test_gpu_shake_standalone.py).  The words left unsynchronised are sample / state values, never an index or a loop
          bound, and every thread still takes the same number of barriers: wrong samples, no fault and no hang.
"""
import os
from concurrent.futures import ThreadPoolExecutor

from audiblelight_amd import _build

ROOT = _build.ROOT
OUT = os.path.join(ROOT, "tests", "shake_build")
VARIANTS = {
    "s1": ["-DAL_SHAKE=1"],
    "s3w": ["-DAL_SHAKE=3", "-DAL_Q16_WAVES=1", "-DAL_SPLIT_WAVES=2"],
    "revert": ["-DAL_SHAKE=3", "-DAL_TEST_REVERT_Q16_BARRIER=1", "-DAL_TEST_REVERT_SOS_BARRIER=1", "-DAL_TEST_REVERT_DELAY_BARRIER=1"],
}
# further skews, built on demand only (profiles/tools/shake_diag.py s2 s4 s5 s6: a wider sweep than the test suite's two variants)
EXTRA_VARIANTS = {
    "s2": ["-DAL_SHAKE=2"],
    "s4": ["-DAL_SHAKE=4"],                      # wave 0 always the FIRST to move on
    "s5": ["-DAL_SHAKE=5", "-DAL_Q16_WAVES=1"],
    "s6": ["-DAL_SHAKE=6", "-DAL_SPLIT_WAVES=2"],
}


def library_path(name: str) -> str:
    return os.path.join(OUT, f"libaudiblelight_hip_{name}.so")


def build(names=None) -> dict:
    """Compile the named variants (default: all) with hipcc for gfx950; returns {name: path}.  Needs no GPU.  Every variant is the
    product recipe (audiblelight_amd/_build.py) plus its defines, all of them side by side over one planner object."""
    names = list(VARIANTS) if names is None else list(names)
    deps = _build.dependencies() + [os.path.abspath(__file__), os.path.abspath(_build.__file__)]
    todo = [name for name in names if _build.stale(library_path(name), deps)]
    if todo:
        os.makedirs(OUT, exist_ok=True)
        plan_obj = os.path.join(OUT, "al_plan.o")
        if _build.compile_planner(plan_obj).wait() != 0:
            raise RuntimeError("g++ failed on the planner")
        defines = {**VARIANTS, **EXTRA_VARIANTS}
        with ThreadPoolExecutor(len(todo)) as pool:
            for objs in pool.map(lambda name: _build.compile_library(library_path(name), defines[name], "_" + name, plan_obj), todo):
                for o in objs:
                    os.remove(o)
    return {name: library_path(name) for name in names}


def existing_or_built(names) -> dict:
    """The variants as __graft_entry__.build() left them in the tree (they travel to the GPU box with it; file times may not), compiled
    only where one is missing."""
    missing = [n for n in names if not os.path.exists(library_path(n))]
    if missing:
        build(missing)
    return {n: library_path(n) for n in names}
