"""fp30s.hip.h / g1_30s.hip.h under UndefinedBehaviorSanitizer: a stand-alone host program (its own main, nothing
preloaded) compiled with -fsanitize=signed-integer-overflow,undefined -fno-sanitize-recover=all runs the model's
worst-case limb patterns through mul, sqr and mul2, lazy limbs at +-3 * 2^29 through the carry pass, and 10^5 random
additions of g1s::chain_add (random table slots and signs, a restart from empty every 64 additions, a repeated slot
now and then so that the tangent and the cancellation run too, every sum taken back through to_xyzz28).  It must exit
clean: the column sums are kept in unsigned arithmetic and everything else is bounded (tests/fp30s_model.py), so no
signed operation may overflow."""
import os
import shutil
import subprocess

import pytest

import fp30s_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include <cstdint>
#include "g1_30s.hip.h"
using fp30s::Fe;
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static fp28::Fe slot() {  // a canonical-looking table coordinate: normalized limbs, value below p
    fp28::Fe r;
    for (int i = 0; i < 13; ++i) r.v[i] = (uint32_t)rnd() & fp28::MASK;
    r.v[13] = (uint32_t)(rnd() % 0x1a011);
    return r;
}
int main() {
    const fp30s::Seeds sd = fp30s::seeds();
    int32_t t[4][13];
    unsigned sink = 0;
    char op[8];
    while (scanf("%7s", op) == 1) {
        const int n = op[0] == 's' ? 1 : op[0] == 'c' ? 1 : op[3] == '2' ? 4 : 2;
        Fe f[4];
        for (int k = 0; k < n; ++k)
            for (int i = 0; i < 13; ++i) { if (scanf("%d", &t[k][i]) != 1) return 2; f[k].v[i] = t[k][i]; }
        const Fe r = op[0] == 's' ? fp30s::sqr(f[0], sd) : op[0] == 'c' ? fp30s::carry(f[0]) : n == 4 ? fp30s::mul2(f[0], f[1], f[2], f[3], sd) : fp30s::mul(f[0], f[1], sd);
        sink += (unsigned)r.v[0] + fp30s::is_zero_mod_p(r);
    }
    g1s::Xyzz acc;
    g1s::set_inf(acc);
    ff::u32 st = g1::CHAIN_EMPTY;
    fp28::Fe px = slot(), py = slot();
    for (int it = 0; it < 100000; ++it) {
        if (it % 64 == 0) { g1s::set_inf(acc); st = g1::CHAIN_EMPTY; }
        if (it % 97 > 2) { px = slot(); py = slot(); }  // else the slot of the addition before: P + P, P - P
        g1s::chain_add(acc, st, px, py, (rnd() & 1) ? 0xffffffffu : 0u, sd);
        if (it % 8 == 7) { g1::Xyzz out; g1s::to_xyzz28(out, acc, st, sd); sink += out.x.v[0] + out.zzz.v[13]; }
    }
    printf("done %u\n", sink);
    return 0;
}
'''


def test_no_undefined_behaviour_on_the_worst_cases_and_on_random_additions(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++")
    src = tmp_path / "fp30s_ubsan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "fp30s_ubsan"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)]
    # whether the sanitizer can be used at all is decided on an empty program with the same flags: only that may skip.
    # Every failure to build the real program fails the test.
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(cmd[:-3] + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (probed.stderr.strip().split("\n") or [""])[-1])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    H = M.H
    lines = []
    for kind, ops, _ in M.worst_case_products():
        lines.append({"mul": "mul", "mul_u": "mul", "sqr": "sqr", "mul2": "mul2"}[kind] + " " + " ".join(str(v) for o in ops for v in o))
    for sign in (1, -1):
        for top in (-(1 << 25), 1 << 25):
            lines.append("carry " + " ".join(str(v) for v in [sign * 3 * H] * 12 + [top]))
    assert len(lines) > 40
    run = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("done") and "runtime error" not in run.stderr, run.stderr[-2000:]
