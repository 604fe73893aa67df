"""Builds and runs tests/device_checks/lane_check.hip for the lane-arithmetic tests (the GPU module and the
cross-compilation check of the CPU module).  The compiler and the flags are the product's, from rust-kzg_amd/build.py."""
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


def product_build():
    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_command(out, defines):
    b = product_build()
    return [b.hipcc_path()] + list(b.COMPILE_FLAGS) + list(defines) + ["-I", CSRC, SOURCE, "-o", out]


def compile_all(outdir, define_sets):
    """name -> executable; the compilations run side by side (a device compilation of these headers is one thread)"""
    procs = {}
    for name, defines in define_sets.items():
        out = os.path.join(str(outdir), "lane_check_" + name)
        procs[name] = (out, subprocess.Popen(compile_command(out, defines), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    built, errors = {}, {}
    for name, (out, p) in procs.items():
        log, _ = p.communicate()
        if p.returncode == 0 and os.path.exists(out):
            built[name] = out
        else:
            errors[name] = log[-4000:]
    return built, errors
