"""THE build recipe of the HIP library: translation units, per-unit flags, dependencies and the one compile function.

``__graft_entry__.build()`` compiles the product library from it, ``tests/shake.py`` the schedule-perturbed variants (the same
call plus ``-D`` defines, so a variant is the product recipe plus its defines by construction), ``tests/hostemu`` takes the unit
and dependency lists for its g++ build.  Imports nothing but the standard library: no torch, no GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audiblelight_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "audiblelight_hip.h")
# device translation units with their own flags: the FFT kernels lose 10-25 % to SLP vectorisation, the spectral MAC gains from it
# (head comment of csrc/al_transforms.hip)
DEVICE_UNITS = (("al_kernels.hip", ()), ("al_transforms.hip", ("-fno-slp-vectorize",)))
PLANNER = "al_plan.cpp"   # the host-side planner behind the same C ABI: plain C++, no device code
PLANNER_CXX = ("g++", "-O2", "-std=c++17", "-fPIC", "-Wall")


def sources():
    """The device units and the planner, as paths."""
    return [os.path.join(CSRC, unit) for unit, _ in DEVICE_UNITS] + [os.path.join(CSRC, PLANNER)]


def dependencies():
    """Every file a library built from this recipe depends on."""
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".cpp"))] + [HEADER]


def stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def compile_planner(obj):
    """The planner's object file, as a running process."""
    return subprocess.Popen([*PLANNER_CXX, "-c", os.path.join(CSRC, PLANNER), "-o", obj])


def compile_library(out, defines=(), tag="", planner_obj=None):
    """hipcc --offload-arch=gfx950: the device units (side by side) and the planner, with ``defines`` on the device units, linked into
    ``out``.  The object files land beside ``out`` as <unit><tag>.o and are returned; ``planner_obj``: one that exists already."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj_dir = os.path.dirname(out)
    os.makedirs(obj_dir, exist_ok=True)
    objs, jobs = [], []
    for unit, flags in DEVICE_UNITS:
        objs.append(os.path.join(obj_dir, os.path.splitext(unit)[0] + tag + ".o"))
        jobs.append(subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", *flags, *defines,
                                      os.path.join(CSRC, unit), "-o", objs[-1]]))
    if planner_obj is None:
        planner_obj = os.path.join(obj_dir, os.path.splitext(PLANNER)[0] + ".o")
        jobs.append(compile_planner(planner_obj))
    if any(job.wait() != 0 for job in jobs):
        raise RuntimeError(f"hipcc failed on {os.path.basename(out)}")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, planner_obj, "-o", out])
    return objs
