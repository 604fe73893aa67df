"""Builds the test-only device harnesses under tests/device_checks/ — lane_check.hip for the lane-arithmetic tests,
fr_check.hip for the Fr arithmetic of the NTT, g2_check.hip for the Fp2 / G2 arithmetic that holds one value per lane
(g2_28.hip.h, g2_io.hip.h, g2_lincomb.hip.h) and the fp28.hip.h primitives under it — for the GPU modules and the
cross-compilation checks of the CPU modules.  The compiler and the flags are the product's, from rust-kzg_amd/build.py.
g2_check.hip and fr_check.hip also have a host form (host_compile_command: any C++17 compiler, no HIP)."""
import shutil
import importlib.util
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg_amd", "csrc")
SOURCE = os.path.join(HERE, "device_checks", "lane_check.hip")

# the builds the GPU module holds to the model, and the one whose planted errors the checkers must find
DEFINE_SETS = {"product": [], "exact": ["-DKZGAMD_FORCE_EXACT_TESTS"], "digit_ahead": ["-DKZGAMD_WMUL_DIGIT_AHEAD"]}
PLANTED = {"planted": ["-DLANE_CHECK_PLANT_ERROR"]}

# fr_check.hip: the product's form, mul_signed without the opaque accumulator chain (the form tools/ instantiate), and
# the planted errors
FR_SOURCE = os.path.join(HERE, "device_checks", "fr_check.hip")
FR_DEFINE_SETS = {"product": [], "unchained": ["-DFR_CHECK_UNCHAINED"]}
FR_PLANTED = {"planted": ["-DFR_CHECK_PLANT_ERROR"]}

# g2_check.hip: the product's form, the exact zero test without its filter (every addition takes the other branch),
# and the planted errors
G2_SOURCE = os.path.join(HERE, "device_checks", "g2_check.hip")
G2_DEFINE_SETS = {"product": [], "exact": ["-DKZGAMD_FORCE_EXACT_TESTS"]}
G2_PLANTED = {"planted": ["-DG2_CHECK_PLANT_ERROR"]}


def product_build():
    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_command(out, defines, source=SOURCE):
    b = product_build()
    return [b.hipcc_path()] + list(b.COMPILE_FLAGS) + list(defines) + ["-I", CSRC, source, "-o", out]


def compile_all(outdir, define_sets, source=SOURCE):
    """name -> executable; the compilations run side by side (a device compilation of these headers is one thread)"""
    procs = {}
    stem = os.path.splitext(os.path.basename(source))[0]
    for name, defines in define_sets.items():
        out = os.path.join(str(outdir), stem + "_" + name)
        procs[name] = (out, subprocess.Popen(compile_command(out, defines, source), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    built, errors = {}, {}
    for name, (out, p) in procs.items():
        log, _ = p.communicate()
        if p.returncode == 0 and os.path.exists(out):
            built[name] = out
        else:
            errors[name] = log[-4000:]
    return built, errors


def host_compile_command(out, defines, source=G2_SOURCE, host_define="-DG2_CHECK_HOST"):
    """the harness's host form: the same op bodies in a plain loop over cases"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    return [cxx, "-O1", "-std=c++17", "-x", "c++", host_define, "-Wno-unknown-pragmas"] + list(defines) + ["-I", CSRC, source, "-o", out]
