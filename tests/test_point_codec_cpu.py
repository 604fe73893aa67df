"""g2_io.hip.h (the G2 wire format, the Fp2 square root, the sign rule and the psi membership test, one value per lane),
the new pairing::g2_in_g2 of host_pairing.h and the chunked G1 lane code of g1_io.hip.h, compiled for the host in one
stand-alone program (its own main) and held to each other and to tests/codec_model.py (Python integers):

  U  every entry of tests/g2_encodings.py: g2io::uncompress == pairing::g2_uncompress (verdict and point), the verdicts
     == the catalogue's class, g2io::in_g2 == g2_in_g2 (psi) == g2_in_g2_by_order ([r]P) == the model, and the point
     re-encoded by g2io::compress == pairing::g2_compress == the input bytes;
  C  random points of G2, of small order and of full order with a random Z, and identities with junk in X and Y:
     g2io::compress == pairing::g2_compress == the model's bytes, membership as above;
  L  lex_largest at c1 = 0 with c0 in {0, 1, (p-1)/2, (p+1)/2, p-1} and at c1 in {1, (p-1)/2, (p+1)/2, p-1};
  S  sqrt on squares, non-squares, 0, purely real and purely imaginary values, with every component at the top of the
     documented bound (63 p on top of the residue) as well: found == the norm criterion == f2_sqrt, root^2 == a, root
     normalized and below 2p;
  K  the psi constants of the header == the model's (powers of 1 + u);
  G  g1io::jac_chunk_out with chunks of 1, 4, 8 and 16 against host_p1_compress_batch / host_p1_to_affine_batch on
     runs of points that leave chunks with no, one and only identities, and an empty chunk that must write nothing.

The same program is built once more under UndefinedBehaviorSanitizer and run on the same script (nothing preloaded),
and codec.hip must cross-compile for gfx950 with the product's flags."""
import importlib.util
import os
import random
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-kzg_amd", "csrc")
sys.path.insert(0, HERE)
import codec_model as M  # noqa: E402
import g1_encodings as E1  # noqa: E402
import g2_encodings as E2  # noqa: E402

P = M.P
M28 = (1 << 28) - 1
R392 = 1 << 392
R384 = 1 << 384

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "g2_io.hip.h"
#include "host_pairing.h"
namespace hp = kzgamd::pairing;
using fp28::Fe;
using g2::F2;
static bool rd_fp(ff::Fp& r) {  // 96 hex digits, big-endian
    char s[128];
    if (scanf("%120s", s) != 1 || strlen(s) != 96) return false;
    for (int i = 0; i < 12; ++i) { unsigned v; if (sscanf(s + (11 - i) * 8, "%8x", &v) != 1) return false; r.v[i] = v; }
    return true;
}
static bool rd_bytes(unsigned char* b, int n) {
    char s[256];
    if (scanf("%250s", s) != 1 || (int)strlen(s) != 2 * n) return false;
    for (int i = 0; i < n; ++i) { unsigned v; if (sscanf(s + 2 * i, "%2x", &v) != 1) return false; b[i] = (unsigned char)v; }
    return true;
}
static bool rd(Fe& r) { for (int i = 0; i < 14; ++i) if (scanf("%x", &r.v[i]) != 1) return false; return true; }
static void raw(const Fe& a) { for (int i = 0; i < 14; ++i) printf("%x ", a.v[i]); }
static void hex(const unsigned char* b, int n) { for (int i = 0; i < n; ++i) printf("%02x", b[i]); }
static hp::Fp2 spec(const F2& a) { ff::Fp o[2]; g2::to_blst(o, a); return {o[0], o[1]}; }
static hp::G2Jac jac_of(const g2::AffPt& a) {
    if (a.flags & 1) return hp::g2_inf();
    return {spec(a.x), spec(a.y), hp::f2_one()};
}
static bool same(const hp::G2Jac& a, const hp::G2Jac& b) { return hp::f2_eq(a.x, b.x) && hp::f2_eq(a.y, b.y) && hp::f2_eq(a.z, b.z); }
template <int CH>
static bool chunks_agree(const std::vector<ff::Fp>& jac, int m, const unsigned char* want48, const ff::Fp* want_aff) {
    std::vector<unsigned char> out(48 * m + 48, 0xa5);
    std::vector<ff::Fp> aff(2 * m + 2);
    memset(aff.data(), 0xa5, aff.size() * sizeof(ff::Fp));
    for (int at = 0; at < m; at += CH) {
        const int c = m - at < CH ? m - at : CH;
        g1io::jac_chunk_out<CH, false>(out.data() + 48 * at, jac.data() + 3 * at, c);
        g1io::jac_chunk_out<CH, true>(aff.data() + 2 * at, jac.data() + 3 * at, c);
    }
    g1io::jac_chunk_out<CH, false>(out.data() + 48 * m, jac.data(), 0);  // an empty chunk writes nothing
    g1io::jac_chunk_out<CH, true>(aff.data() + 2 * m, jac.data(), 0);
    bool ok = !memcmp(out.data(), want48, 48 * m) && !memcmp(aff.data(), want_aff, 2 * m * sizeof(ff::Fp));
    for (int k = 0; k < 48; ++k) ok = ok && out[48 * m + k] == 0xa5;
    for (size_t k = 0; k < 2 * sizeof(ff::Fp); ++k) ok = ok && ((unsigned char*)(aff.data() + 2 * m))[k] == 0xa5;
    return ok;
}
int main() {
    char op[16];
    while (scanf("%15s", op) == 1) {
        if (op[0] == 'U') {
            unsigned char in[96], re[96] = {0}, hre[96];
            if (!rd_bytes(in, 96)) return 2;
            g2::AffPt a;
            hp::G2Jac h;
            const bool dok = g2io::uncompress(a, in), hok = hp::g2_uncompress(h, in);
            bool agree = dok == hok;
            int dev_in = -1, h_psi = -1, h_ord = -1;
            if (dok && hok) {
                const hp::G2Jac d = jac_of(a);
                agree = agree && same(d, h);
                dev_in = g2io::in_g2(a);
                h_psi = hp::g2_in_g2(h);
                h_ord = hp::g2_in_g2_by_order(h);
                g2::Jac j;
                g2::from_blst_jacobian(j, reinterpret_cast<const ff::Fp*>(&d));
                g2io::compress(re, j);
                hp::g2_compress(hre, h);
                agree = agree && !memcmp(re, hre, 96);
            }
            printf("%d %d %d %d %d ", (int)dok, dev_in, h_psi, h_ord, (int)agree);
            hex(re, 96);
            printf("\n");
        } else if (op[0] == 'C') {
            ff::Fp c[6];
            for (int i = 0; i < 6; ++i) if (!rd_fp(c[i])) return 2;
            hp::G2Jac h;
            memcpy(&h, c, sizeof h);
            g2::Jac j;
            g2::from_blst_jacobian(j, c);
            unsigned char re[96], hre[96];
            g2io::compress(re, j);
            hp::g2_compress(hre, h);
            g2::AffPt a;
            g2::to_affine(a, j);
            printf("%d %d %d %d ", (int)g2io::in_g2(a), (int)hp::g2_in_g2(h), (int)hp::g2_in_g2_by_order(h), (int)!memcmp(re, hre, 96));
            hex(re, 96);
            printf("\n");
        } else if (op[0] == 'L') {
            ff::Fp c0, c1;
            if (!rd_fp(c0) || !rd_fp(c1)) return 2;
            const F2 y = {g1io::from_plain(c0), g1io::from_plain(c1)};
            const hp::Fp2 hy = {hfp::to_mont(c0), hfp::to_mont(c1)};
            printf("%d %d\n", (int)g2io::lex_largest(y), (int)hp::f2_lex_largest(hy));
        } else if (op[0] == 'S') {
            F2 a, r;
            if (!rd(a.c0) || !rd(a.c1)) return 2;
            hp::Fp2 hr;
            const bool hf = hp::f2_sqrt(hr, spec(a));
            const bool f = g2io::sqrt(r, a);
            printf("%d %d ", (int)f, (int)hf);
            raw(r.c0);
            raw(r.c1);
            printf("\n");
        } else if (op[0] == 'K') {
            raw(g2io::psi_x().c0); raw(g2io::psi_x().c1); raw(g2io::psi_y().c0); raw(g2io::psi_y().c1);
            printf("\n");
        } else if (op[0] == 'G') {
            int m;
            if (scanf("%d", &m) != 1 || m < 0 || m > 4096) return 2;
            std::vector<ff::Fp> jac(3 * m + 3);
            for (int i = 0; i < 3 * m; ++i) if (!rd_fp(jac[i])) return 2;
            std::vector<unsigned char> want(48 * m + 1);
            std::vector<ff::Fp> aff(2 * m + 1);
            const blst_p1* pts = reinterpret_cast<const blst_p1*>(jac.data());
            kzgamd::host_p1_compress_batch(want.data(), pts, m);
            kzgamd::host_p1_to_affine_batch(aff.data(), m, [&](size_t i) { return pts + i; });
            printf("%d %d %d %d ", (int)chunks_agree<1>(jac, m, want.data(), aff.data()), (int)chunks_agree<4>(jac, m, want.data(), aff.data()),
                   (int)chunks_agree<8>(jac, m, want.data(), aff.data()), (int)chunks_agree<16>(jac, m, want.data(), aff.data()));
            hex(want.data(), 48 * m);
            printf("\n");
        } else return 4;
    }
    return 0;
}
'''


def limbs(v):
    assert 0 <= v < 1 << 392
    return [(v >> (28 * i)) & M28 for i in range(13)] + [v >> 364]


def value(l):
    return sum(x << (28 * i) for i, x in enumerate(l))


def fe(v):
    return " ".join("%x" % x for x in limbs(v))


def h96(v):
    assert 0 <= v < 1 << 384
    return "%096x" % v


def mont(v):
    return h96(v * R384 % P)


def g2_jacobian(a, z, junk=None):
    """the six blst_p2 words of the affine point a over this Z (None: the identity, with `junk` in X and Y)"""
    if a is None:
        return [mont(c) for c in (junk or (0, 0, 0, 0))] + [h96(0), h96(0)]
    z2 = M.f2sqr(z)
    x, y = M.f2mul(a[0], z2), M.f2mul(a[1], M.f2mul(z2, z))
    return [mont(c) for c in x + y + tuple(z)]


def g1_jacobian(a, z, junk=(0, 0)):
    if a is None:
        return [mont(junk[0]), mont(junk[1]), h96(0)]
    return [mont(a[0] * z * z % P), mont(a[1] * z * z * z % P), mont(z)]


class Script:
    def __init__(self):
        self.lines, self.checks = [], []

    def add(self, line, *check):
        self.lines.append(line)
        self.checks.append(check)


def build_script(rnd):
    s = Script()
    s.add("K", "K")
    for name, b, cls in E2.catalogue():
        s.add("U " + b.hex(), "U", name, b, cls)
    # points with a random Z: G2, small order, full order, identities with junk
    tors = [M.torsion_point(q) for q in M.small_cofactor_primes()[:3]]
    full = [M.point_with_x((c0, 0), 0) for c0 in range(1, 12)]
    pool = [M.mul(rnd.randrange(1, M.R), M.G2) for _ in range(8)] + tors + [a for a in full if a is not None][:3]
    pool.append(M.add(tors[0], pool[0]))
    for a in pool:
        for z in ((1, 0), (rnd.randrange(1, P), rnd.randrange(P)), (0, rnd.randrange(1, P))):
            s.add("C " + " ".join(g2_jacobian(a, z)), "C", a)
    for _ in range(3):
        s.add("C " + " ".join(g2_jacobian(None, None, [rnd.randrange(P) for _ in range(4)])), "C", None)
    s.add("C " + " ".join(g2_jacobian(None, None)), "C", None)
    # the sign rule
    half = (P - 1) // 2
    for c0 in (0, 1, half, half + 1, P - 1):
        s.add("L %s %s" % (h96(c0), h96(0)), "L", (c0, 0))
    for c1 in (1, half, half + 1, P - 1):
        for c0 in (0, 1, half, half + 1, P - 1, rnd.randrange(P)):
            s.add("L %s %s" % (h96(c0), h96(c1)), "L", (c0, c1))
    # square roots
    vals = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1), (4, 0), (0, 4), (P - 4, 0), (2, 0), (0, 2), (3, 0), (5, 0), (0, 3)]
    for _ in range(16):
        r = (rnd.randrange(P), rnd.randrange(P))
        vals += [M.f2sqr(r), (r[0], 0), (0, r[1]), (rnd.randrange(P), rnd.randrange(P)), (r[0] * r[0] % P, 0), (-r[0] * r[0] % P, 0)]
    for a in vals:
        for k in (0, 1, 63):
            s.add("S %s %s" % (fe(a[0] * R392 % P + k * P), fe(a[1] * R392 % P + k * P)), "S", a)
    # the chunked G1 lane code: Z = 1, random Z, identities with junk, so that chunks hold no, one and only identities
    g1 = [E1.mul(rnd.randrange(1, E1.R), E1.G) for _ in range(6)]

    def run_of(pattern):
        out = []
        for i, c in enumerate(pattern):
            if c == "o":
                out += g1_jacobian(None, None, (rnd.randrange(P), rnd.randrange(P)))
            else:
                out += g1_jacobian(g1[i % len(g1)], 1 if c == "1" else rnd.randrange(1, P))
        return out

    for pattern in ("", "z", "o", "1", "zzzz" + "oooo" + "ozoo" + "zzoz" + "o", "o" * 16 + "z" * 16 + "oooooooz" + "zooooooo" + "1z",
                    "o" * 33, "z" * 17, "zo" * 20):
        want = b"".join(E1.compress(None) if c == "o" else E1.compress(g1[i % len(g1)]) for i, c in enumerate(pattern))
        s.add("G %d %s" % (len(pattern), " ".join(run_of(pattern))), "G", want)
    return s


def check_output(s, out):
    lines = out.strip("\n").split("\n")
    assert len(lines) == len(s.checks) > 300
    seen = {0: 0, 1: 0, 2: 0}
    rinv = pow(R392, -1, P)
    for chk, ln in zip(s.checks, lines):
        t = ln.split()
        if chk[0] == "K":
            v = [int(x, 16) for x in t]
            cx, cy = M.psi_constants()
            assert v[0:14] == M.limbs28(cx[0]) == [0] * 14 and v[14:28] == M.limbs28(cx[1]), "psi constant of x"
            assert v[28:42] == M.limbs28(cy[0]) and v[42:56] == M.limbs28(cy[1]), "psi constant of y"
        elif chk[0] == "U":
            _, name, b, cls = chk
            dok, dev_in, h_psi, h_ord, agree = (int(x) for x in t[:5])
            assert agree == 1, "%s: g2_io.hip.h and host_pairing.h differ" % name
            assert dok == (cls != 1), "%s: decoded %d, class %d" % (name, dok, cls)
            if dok:
                assert dev_in == h_psi == h_ord == (1 if cls == 0 else 0), (name, dev_in, h_psi, h_ord, cls)
                assert bytes.fromhex(t[5]) == b, "%s: does not re-encode to itself" % name
            seen[cls] += 1
        elif chk[0] == "C":
            a = chk[1]
            member = 1 if M.in_g2(a) else 0
            assert [int(x) for x in t[:4]] == [member, member, member, 1], (a, t[:4])
            assert bytes.fromhex(t[4]) == M.compress(a)
        elif chk[0] == "L":
            want = 1 if M.lex_largest(chk[1]) else 0
            assert [int(x) for x in t] == [want, want], chk[1]
        elif chk[0] == "S":
            a = chk[1]
            found, host_found = int(t[0]), int(t[1])
            assert found == host_found == (1 if M.f2_is_square(a) else 0), a
            comps = [[int(x, 16) for x in t[2 + 14 * k:16 + 14 * k]] for k in range(2)]
            for c in comps:
                assert all(x <= M28 for x in c[:13]) and value(c) < 2 * P, "sqrt: not normalized below 2p"
            if found:
                r = tuple(value(c) * rinv % P for c in comps)
                assert M.f2sqr(r) == a, "sqrt: not a root"
            else:
                assert all(x == 0 for c in comps for x in c)
        elif chk[0] == "G":
            assert t[:4] == ["1"] * 4, "jac_chunk_out differs from the host batch (chunks of 1, 4, 8, 16): %s" % t[:4]
            assert bytes.fromhex(t[4] if len(t) > 4 else "") == chk[1]
    assert all(v >= 20 for v in seen.values()), seen


def compile_program(tmp_path, name, extra, cxx=None):
    cxx = cxx or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / (name + ".cpp")
    src.write_text(PROGRAM)
    exe = tmp_path / name
    return [cxx, "-O1", "-std=c++17"] + extra + ["-I", CSRC, str(src), "-o", str(exe), "-lpthread"], exe


def test_the_model_pins_itself_and_the_catalogue_has_every_class():
    assert M.self_check()
    assert M.small_cofactor_primes()[:2] == [13, 23]
    cat = E2.catalogue()
    names = " | ".join(n for n, _, _ in cat)
    for need in ("flags 000", "flags 111", "x.c1 = p", "x.c0 = p", "2^381 - 1", "infinity with the sign flag", "not a square",
                 "order 13", "order 13 + G", " u, sign 1"):
        assert need in names, need


@pytest.mark.parametrize("exact", [False, True])
def test_g2_wire_format_and_membership_lane_code_against_host_and_model(tmp_path, exact):
    s = build_script(random.Random(0x6732))
    cmd, exe = compile_program(tmp_path, "codeccheck", ["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else [])
    subprocess.check_call(cmd)
    run = subprocess.run([str(exe)], input="\n".join(s.lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    check_output(s, run.stdout)


def test_no_undefined_behaviour_in_the_codec_lane_code(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++")
    flags = ["-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([cxx, "-O1", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (probed.stderr.strip().split("\n") or [""])[-1])
    cmd, exe = compile_program(tmp_path, "codeccheck_ubsan", flags, cxx)
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    s = build_script(random.Random(0x6732))
    run = subprocess.run([str(exe)], input="\n".join(s.lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and "runtime error" not in run.stderr, run.stderr[-2000:]
    check_output(s, run.stdout)


def test_codec_cross_compiles_for_gfx950_with_the_products_flags(tmp_path):
    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build_codec", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "codec.hip" in b.SOURCES and "g2_io.hip.h" in b.HEADERS
    out = str(tmp_path / "codec.o")
    p = subprocess.run([b.hipcc_path()] + b.COMPILE_FLAGS + ["-fPIC", "-c", os.path.join(CSRC, "codec.hip"), "-o", out],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.getsize(out) > 0, p.stderr[-3000:]
