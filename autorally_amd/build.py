"""Builds libmppi_hip.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

hipcc cross-compiles without a GPU, so this also is the "does it build" check run on CPU.
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmppi_hip.so")
SOURCES = ["mppi_abi.hip", "abi_forms.hip", "abi_pack.hip", "abi_solve.hip", "abi_host.hip", "abi_trace.hip", "rollout_mfma.hip", "rollout_multi.hip", "rollout_oct.hip", "rollout_row.hip", "rollout_row32.hip", "rollout_row64.hip", "rollout_m44.hip", "rollout_lds44.hip", "rollout_lds128.hip", "rollout_lds16.hip", "rollout_fleet16.hip", "rollout_fleet_multi.hip", "rollout_glb16.hip", "rollout_glb44.hip", "rollout_valu.hip", "rollout_trace.hip", "ddp_fleet.hip", "nominal_fleet.hip", "nominal_gains_fleet.hip", "plant_fleet.hip", "plant_drive_fleet.hip", "solve_kernels.hip",
           "noise_mrg32k3a.hip", "rollout_bf.hip", "rollout_fleet_bf.hip", "rollout_bf_row.hip", "ddp_feedback.cpp"]
HEADERS = ["abi_internal.hpp", "mppi_device.hpp", "mfma_net.hpp", "group_roles.hpp", "m44_core.hpp", "m44_group.hpp", "multi_group.hpp", "row_group.hpp", "wave16_step.hpp", "wave16_image.hpp", "mppi_kernels.hpp", "noise_device.hpp", "ddp_feedback.hpp", "basis_funcs.hpp", "bf_device.hpp", "bf_group.hpp", "bf_row_device.hpp", "host_net.hpp", "tanhf_vec.hpp", "tanhf_scalar.hpp", "ddp_fleet_device.hpp", "nominal_fleet_device.hpp", "wave_net.hpp", os.path.join("..", "..", "include", "mppi_hip.h")]
# -ffp-contract=off: every FMA in the kernels is explicit (see csrc/mppi_device.hpp)
# -amdgpu-mfma-vgpr-form: MFMA results land in VGPRs (gfx950 has one unified file), which removes
# the v_accvgpr_read per accumulator register after every layer
# host side: x86-64-v3 (AVX2 + FMA) so that fmaf() in the host replays is one instruction (same
# assumption as oracle/Makefile; every MI355X host CPU has it)
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wall",
         "-Wno-unused-function", "-mllvm", "-amdgpu-mfma-vgpr-form", "-Xarch_host", "-mavx2", "-Xarch_host", "-mfma"]


# per-file additions: the row form's T loop is one wave's dependent chains with their operand moves in the shadow of the
# multiply-adds; the scheduler's max-ILP strategy orders the bookkeeping around them better than the default
# (same-box A/B: 0.0577 -> 0.0569 ms per step, the batched kernel unchanged; the other kernels keep the default)
EXTRA_FLAGS = {"rollout_row.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
               "rollout_row32.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
               "rollout_row64.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]}


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    cc = hipcc()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    # a tree that arrives with the library but without its object files: nothing to do while no source is newer than the library
    if not force and not _stale(LIB, [os.path.join(CSRC, s) for s in SOURCES] + hdrs):
        return LIB
    jobs = []
    objs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s.replace(".hip", ".o").replace(".cpp", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append([cc] + FLAGS + EXTRA_FLAGS.get(s, []) + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr))
        return r.stderr

    with ThreadPoolExecutor(max_workers=4) as ex:
        for warn in ex.map(run, jobs):
            if verbose and warn:
                print(warn, file=sys.stderr)
    if jobs or force or _stale(LIB, objs):
        run([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


HOST = os.path.join(HERE, "host")
BIN = os.path.join(HERE, "bin")


def build_host(force=False):
    """C++ host layer above the C ABI (the reference's controller surface, ROS-free binary).
    Plain g++: the host code only sees include/mppi_hip.h and links libmppi_hip.so."""
    os.makedirs(BIN, exist_ok=True)
    cxx = shutil.which("g++") or "g++"
    hdrs = [os.path.join(HOST, h) for h in ("npz.hpp", "param_getter.hpp", "mppi_controller_hip.hpp",
                                            "run_control_loop.hpp", "path_integral_main.hpp")] + [os.path.join(CSRC, h) for h in ("basis_funcs.hpp", "host_net.hpp", "tanhf_vec.hpp")] + [os.path.join(HERE, "..", "include", "mppi_hip.h")]
    outs = []
    link = ["-L" + HERE, "-lmppi_hip", "-Wl,-rpath,$ORIGIN/.."]
    for name, libs in (("host_selftest", link), ("path_integral_nn", link), ("path_integral_bf", link)):
        src = os.path.join(HOST, name + ".cpp")
        out = os.path.join(BIN, name)
        outs.append(out)
        if force or _stale(out, [src] + hdrs + ([LIB] if libs else [])):
            cmd = [cxx, "-O2", "-mavx2", "-mfma", "-ffp-contract=off", "-std=c++17", "-Wall", "-DMPPI_NPZ_ZLIB", src, "-o", out] + libs + ["-lz", "-lpthread"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("host build failed:\n%s\n%s" % (" ".join(cmd), r.stderr))
    return outs


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_host(force="--force" in sys.argv))
