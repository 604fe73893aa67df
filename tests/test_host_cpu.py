"""CPU-side checks (run with -m "not gpu"): the C-ABI library loads and exports every declared
symbol (no compute calls), the header and the Python mirror agree, the sharding logic works
across 2 ranks (gloo), and the product refuses to run without a GPU instead of falling back."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set()
    for m in re.finditer(r"^[A-Za-z_][\w\s\*]*?\b([a-z_][a-z0-9_]*)\s*\(", src, flags=re.M):
        names.add(m.group(1))
    return names - {"defined"}


def test_library_exports_every_header_symbol(kzg):
    if not os.path.exists(kzg.LIB_PATH):
        import importlib.util

        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build()
    L = C.CDLL(kzg.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 25
    missing = [s for s in sorted(syms) if not hasattr(L, s)]
    assert not missing, missing
    # the Python mirror binds exactly what the header declares
    assert set(kzg.EXPORTS) == syms, (set(kzg.EXPORTS) ^ syms)


def test_struct_layouts_match_reference_abi(kzg):
    # kzg/src/eth/c_bindings.rs:429-474 sizes; CKZGSettings = 8 pointers + 2 usize
    assert C.sizeof(kzg.BlstFr) == 32 and C.sizeof(kzg.BlstFp) == 48
    assert C.sizeof(kzg.BlstP1Affine) == 96 and C.sizeof(kzg.BlstP1) == 144
    assert C.sizeof(kzg.CKZGSettings) == 80
    assert C.sizeof(kzg.RustError) == 16


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the no-GPU behaviour is not observable here")
def test_no_gpu_means_failure_not_fallback(kzg, trusted_setup_text):
    import tempfile

    assert kzg.device_count() == 0
    pts = (kzg.BlstP1Affine * 8)()
    with pytest.raises(kzg.KzgAmdError):
        kzg.prepare_multi_scalar_mult(pts, 8)
    sc = (kzg.BlstFr * 8)()
    with pytest.raises(kzg.KzgAmdError):
        kzg.multi_scalar_mult(pts, sc, 8)
    with pytest.raises(kzg.KzgAmdError):
        kzg.FFTSettings(4)
    with tempfile.NamedTemporaryFile("wb", suffix=".txt") as f:
        f.write(trusted_setup_text)
        f.flush()
        with pytest.raises(kzg.KzgAmdError):
            kzg.KZGSettings.from_file(f.name)


def test_product_sources_never_touch_the_oracle():
    # the oracle is test infrastructure: nothing under rust-kzg_amd/ may include, link or import it
    bad = []
    for dp, _, files in os.walk(os.path.join(ROOT, "rust-kzg_amd")):
        for fn in files:
            if fn.endswith((".so", ".o", ".pyc")):
                continue
            txt = open(os.path.join(dp, fn), errors="ignore").read()
            if re.search(r"oracle[_/\.]|liboracle|oracle_ffi", txt):
                bad.append(os.path.join(dp, fn))
    assert not bad, bad


def test_shard_range_partitions():
    from importlib import util

    spec = util.spec_from_file_location("sharding", os.path.join(ROOT, "rust-kzg_amd", "sharding.py"))
    sh = util.module_from_spec(spec)
    spec.loader.exec_module(sh)
    for n in (0, 1, 7, 8, 255, 256, 257):
        for world in (1, 2, 3, 8):
            spans = [sh.shard_range(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


WORKER = r'''
import ctypes as C, os, sys, random
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch.distributed as dist
from importlib import util
spec = util.spec_from_file_location("sharding", os.path.join(ROOT, "rust-kzg_amd", "sharding.py"))
sh = util.module_from_spec(spec); spec.loader.exec_module(sh)
import oracle_ffi as O
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % PORT, rank=RANK, world_size=2)
with open(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"), "rb") as f:
    rc, s = O.load_settings(f.read())
assert rc == 0
rnd = random.Random(3)
blobs = []
for _ in range(5):
    b = bytearray(rnd.randbytes(131072))
    for i in range(0, 131072, 32):
        b[i] = 0
    blobs.append(bytes(b))
calls = []
def engine(bs):
    calls.append(len(bs))
    out = []
    for b in bs:
        o = C.create_string_buffer(48)
        assert O.lib().oblob_to_kzg_commitment(o, b, C.byref(s)) == 0
        out.append(o.raw)
    return out
got = sh.commit_sharded(blobs, engine, dist)
lo, hi = sh.shard_range(5, 2, RANK)
assert calls == [hi - lo], calls            # each rank computed only its slab
full = engine(blobs)
assert got == full
# the tensor form of the gather (what runs as ncclAllGather on GPUs): uneven slabs, batch order restored
import torch
mine = torch.frombuffer(bytearray(b"".join(full[lo:hi])), dtype=torch.uint8)
allres = sh.gather_results(mine, 5, 48, dist)
assert bytes(allres.numpy().tobytes()) == b"".join(full)
dist.barrier()
dist.destroy_process_group()
print("rank", RANK, "ok")
'''


def test_sharded_commit_two_ranks_gloo(tmp_path):
    # N > 1 path on CPU: world_size 2 over gloo; the per-rank engine is the CPU oracle here
    port = 29500 + (os.getpid() % 500)
    procs = []
    for rank in range(2):
        code = "ROOT=%r\nPORT=%d\nRANK=%d\n" % (ROOT, port, rank) + WORKER
        procs.append(subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for rank, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert "rank %d ok" % rank in o


MSM_WORKER = r'''
import ctypes as C, os, sys, random, importlib.util
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch.distributed as dist
from importlib import util
spec = util.spec_from_file_location("sharding", os.path.join(ROOT, "rust-kzg_amd", "sharding.py"))
sh = util.module_from_spec(spec); spec.loader.exec_module(sh)
path = os.path.join(ROOT, "rust-kzg_amd", "__init__.py")
spec = importlib.util.spec_from_file_location("rust_kzg_amd", path, submodule_search_locations=[os.path.dirname(path)])
kzg = importlib.util.module_from_spec(spec); sys.modules["rust_kzg_amd"] = kzg; spec.loader.exec_module(kzg)
import oracle_ffi as O
L = O.lib()
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % PORT, rank=RANK, world_size=2)
rnd = random.Random(9)
n = 37
g = O.G1(); L.og1_generator(C.byref(g))
pts = (O.G1Affine * n)()
for i in range(n):
    t = O.G1(); k = O.fr_from_int(rnd.randrange(1, O.R))
    L.og1_mul(C.byref(t), C.byref(g), C.byref(k)); L.og1_to_affine(C.byref(pts[i]), C.byref(t))
sc = O.fr_array([rnd.randrange(O.R) for _ in range(n)])
calls = []
def partial(lo, hi):   # the per-rank engine: here the CPU oracle over the slice
    calls.append((lo, hi))
    out = O.G1()
    L.omsm_affine(C.byref(out), C.cast(C.byref(pts, lo * 96), C.POINTER(O.G1Affine)),
                  C.cast(C.byref(sc, lo * 32), C.POINTER(O.Fr)), hi - lo)
    return bytes(out)
got = sh.msm_sharded(n, partial, kzg.g1_sum, dist)   # combine step = the product's host helper
assert calls == [sh.shard_range(n, 2, RANK)], calls
full = O.G1(); L.omsm_affine(C.byref(full), pts, sc, n)
a = O.G1(); C.memmove(C.byref(a), got, 144)
assert L.og1_equal(C.byref(a), C.byref(full)) == 1
# degenerate shapes: fewer points than ranks, and the empty sum
one = sh.msm_sharded(1, partial, kzg.g1_sum, dist)
b = O.G1(); C.memmove(C.byref(b), one, 144)
exp = O.G1(); L.omsm_affine(C.byref(exp), pts, sc, 1)
assert L.og1_equal(C.byref(b), C.byref(exp)) == 1
assert kzg.g1_sum([]) == bytes(144)
dist.barrier()
dist.destroy_process_group()
print("rank", RANK, "ok")
'''


def test_sharded_large_msm_two_ranks_gloo():
    # one large MSM split by index range, partials all-gathered and added with kzgamd_g1_sum
    port = 30100 + (os.getpid() % 500)
    procs = []
    for rank in range(2):
        code = "ROOT=%r\nPORT=%d\nRANK=%d\n" % (ROOT, port, rank) + MSM_WORKER
        procs.append(subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for rank, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert "rank %d ok" % rank in o


def test_prefixed_library_renames_every_ckzg_symbol():
    """libkzg_mi355x_prefixed.so (build.py --prefixed): the c-kzg names are exported as kzgamd_ckzg_* only, everything
    else as in the plain library — what lets a process link the reference's own C bindings next to this one."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    path = b.build_prefixed()
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in b.CKZG_NAMES:
        assert "kzgamd_ckzg_" + n in names and n not in names, n
    assert {"prepare_msm", "mult_pippenger", "ntt_fr", "kzgamd_blob_to_kzg_commitment_device"} <= names
    text = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for n in b.CKZG_NAMES:
        assert "#define %s kzgamd_ckzg_%s" % (n, n) in text, n


def test_fast_field_multipliers_equal_the_generic_ones(tmp_path):
    """hfp::mul (6 x 64-bit limbs, host pairing) and fr29::mul_blst (9 x 29-bit limbs, quotient kernels) are drop-in
    replacements of ff::mul: compiled for the host and compared on random and edge operands."""
    import shutil
    import subprocess

    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++")
    src = tmp_path / "fieldcheck.cpp"
    csrc = os.path.join(ROOT, "rust-kzg_amd", "csrc")
    src.write_text('''
#include <cstdio>
#include <cstdint>
#include "%s/host_fp64.h"
#include "%s/fr29.hip.h"
static uint64_t st = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 16); }
int main() {
    int bad = 0;
    for (int it = 0; it < 20000; ++it) {
        ff::Fp a, b;
        for (int k = 0; k < 12; ++k) { a.v[k] = rnd(); b.v[k] = rnd(); }
        a.v[11] &= 0x0fffffffu; b.v[11] &= 0x0fffffffu;  // below p
        if (it == 0) a = ff::Fp::zero();
        if (it == 1) { a = ff::Fp::modulus(); a.v[0] -= 1; b = a; }
        if (!(hfp::mul(a, b) == ff::mul(a, b))) ++bad;
        if (!(hfp::add(a, b) == ff::add(a, b))) ++bad;
        if (!(hfp::sub(a, b) == ff::sub(a, b))) ++bad;
        ff::Fr x, y;
        for (int k = 0; k < 8; ++k) { x.v[k] = rnd(); y.v[k] = rnd(); }
        x.v[7] &= 0x3fffffffu; y.v[7] &= 0x3fffffffu;  // below r
        if (it == 2) x = ff::Fr::zero();
        if (it == 3) { x = ff::Fr::modulus(); x.v[0] -= 1; y = x; }
        if (!(fr29::mul_blst(x, y) == ff::mul(x, y))) ++bad;
    }
    printf("%%d\\n", bad);
    return bad != 0;
}
''' % (csrc, csrc))
    exe = tmp_path / "fieldcheck"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-x", "c++", str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).strip() == b"0"


def test_batched_binary_gcd_inverse_equals_the_bit_by_bit_one(tmp_path):
    """ff::inverse_plain_fast (30 halving steps per multiword update; the inversion behind every inverse_bgcd call, host
    and device) against ff::inverse_plain_bgcd on edge and random values of Fr and Fp (tools/inv_check.cpp); no call
    may need the fallback."""
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "inv_check"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"),
                           os.path.join(ROOT, "tools", "inv_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe), "60000"]).decode()
    assert "Fr: 0 mismatches" in out and "Fp: 0 mismatches" in out, out
    assert out.count("fallbacks so far 0") == 2, out


def test_dbl_of_a_negated_point_with_a_tiny_y(tmp_path):
    """g1::dbl takes Y up to 8p: the one-lane G1 stage doubles points whose Y is fp28::neg<8>(y) (fftg1.hip: apply_half,
    negated table entries).  With the 8p pad of round 4 the lazy 8p - Y underflowed its top limb whenever the
    Montgomery y was below 8p mod 2^364 (about 9e-6 of all points): directed values with a zero / one top
    limb, negated, doubled, against the same residue reduced below 2p first.  madd / dadd / dadd_unequal get the same
    treatment on their own documented input bounds."""
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "dblcheck.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdint>
#include "g1_28.hip.h"
static uint64_t st = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 16); }
using fp28::Fe;
static Fe rfe(uint32_t top) { Fe r; for (int i = 0; i < 13; ++i) r.v[i] = rnd() & fp28::MASK; r.v[13] = top; return r; }
static bool same(const Fe& a, const Fe& b) { return fp28::to_blst(a) == fp28::to_blst(b); }
static bool same_pt(const g1::Xyzz& a, const g1::Xyzz& b) {  // same representation class: coordinates equal mod p
    return same(a.x, b.x) && same(a.y, b.y) && same(a.zz, b.zz) && same(a.zzz, b.zzz);
}
int main() {
    int bad = 0;
    for (int it = 0; it < 30000; ++it) {
        g1::Xyzz P;
        P.x = rfe(rnd() % 0x1a011);
        P.zz = rfe(rnd() % 0x1a011);
        P.zzz = rfe(rnd() % 0x1a011);
        Fe y = rfe(it % 3 == 0 ? 0 : (it % 3 == 1 ? 1 : rnd() % 0x1a011));
        if (it == 5) y = fp28::zero();
        if (it == 6) for (int i = 0; i < 13; ++i) y.v[i] = fp28::MASK;   // 2^364 - 1
        g1::Xyzz A = P, B = P;
        A.y = fp28::neg<8>(y);                            // 8p - y in (6p, 8p]
        B.y = fp28::mul(fp28::neg<8>(y), fp28::one());    // the same residue, < 2p
        g1::Xyzz A2 = A, B2 = B;
        g1::dbl(A);
        g1::dbl(B);
        if (!same_pt(A, B)) ++bad;
        // the additions with the (6p, 8p] operand on either side (formulas are identities in any field, so the
        // operands need not be curve points)
        g1::Xyzz Q;
        Q.x = rfe(rnd() % 0x1a011); Q.y = rfe(rnd() % 0x1a011); Q.zz = rfe(rnd() % 0x1a011); Q.zzz = rfe(rnd() % 0x1a011);
        g1::Xyzz C = A2, D = B2;
        g1::dadd(C, Q);
        g1::dadd(D, Q);
        if (!same_pt(C, D)) ++bad;
        C = Q; D = Q;
        g1::dadd(C, A2);
        g1::dadd(D, B2);
        if (!same_pt(C, D)) ++bad;
        C = Q; D = Q;
        if (g1::dadd_unequal(C, A2) || g1::dadd_unequal(D, B2)) ++bad;
        if (!same_pt(C, D)) ++bad;
        // madd: accumulator Y below 6p (its documented bound), tiny top limbs included
        g1::Xyzz E = P, F = P;
        E.y = fp28::sub<4>(fp28::addn(y, y), fp28::zero());   // 2y + 4p < 6p
        F.y = fp28::mul(E.y, fp28::one());
        g1::madd(E, Q.x, Q.y);
        g1::madd(F, Q.x, Q.y);
        if (!same_pt(E, F)) ++bad;
    }
    printf("%d\n", bad);
    return bad != 0;
}
''')
    exe = tmp_path / "dblcheck"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), "-x", "c++", str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).strip() == b"0"


def _c_prototypes():
    """{name: [parameter declarations]} of every function include/kzg_mi355x.h declares"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    protos = {}
    for m in re.finditer(r"^[A-Za-z_][\w\s\*]*?\b([a-z_][a-z0-9_]*)\s*\(([^;{]*?)\)\s*;", src, flags=re.M | re.S):
        args = " ".join(m.group(2).split())
        protos[m.group(1)] = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
    return protos


def _rust_externs(path):
    """{name: [parameter declarations]} of every fn inside an extern "C" block of a Rust source"""
    src = open(path).read()
    src = re.sub(r"//.*$", "", src, flags=re.M)
    out = {}
    for block in re.finditer(r'extern\s+"C"\s*\{(.*?)\n\s*\}', src, flags=re.S):
        body = block.group(1)
        for m in re.finditer(r"(#\[link_name\s*=\s*\"(\w+)\"\]\s*)?(?:pub\s+)?fn\s+(\w+)\s*\((.*?)\)\s*(?:->\s*[^;]+)?;", body, flags=re.S):
            args = " ".join(m.group(4).split())
            out[m.group(2) or m.group(3)] = [a.strip() for a in args.split(",") if a.strip()]
    return out


def test_rust_sys_crate_declares_what_the_header_declares():
    """The Rust side of the boundary cannot be compiled in this image (no cargo): at least every `extern "C"` item of the
    sys crate (rust-kzg_amd/rust/src/lib.rs) must name a function of include/kzg_mi355x.h with the same number of
    parameters, pointer parameters where the header has pointers and integers where it has integers, and its #[repr(C)]
    mirror of KzgAmdConfig must have the header's fields in the header's order."""
    protos = _c_prototypes()
    rs = os.path.join(ROOT, "rust-kzg_amd", "rust", "src", "lib.rs")
    ext = _rust_externs(rs)
    assert len(ext) >= 40, sorted(ext)
    for must in ("prepare_msm", "mult_pippenger_prepared", "mult_pippenger", "ntt_fr", "das_fft_extension", "fft_g1",
                 "kzgamd_msm_attach_matrix", "kzgamd_mult_pippenger_matrix", "kzgamd_config_init", "blob_to_kzg_commitment",
                 "compute_cells_and_kzg_proofs", "kzgamd_load_trusted_setup_file_multi"):
        assert must in ext, must
    for name, rargs in ext.items():
        if name == "free":  # libc
            continue
        assert name in protos, "Rust declares %s, the header does not" % name
        cargs = protos[name]
        assert len(rargs) == len(cargs), (name, rargs, cargs)
        for ra, ca in zip(rargs, cargs):
            c_is_ptr = "*" in ca or "[" in ca
            r_is_ptr = "*const" in ra or "*mut" in ra or "&" in ra
            assert c_is_ptr == r_is_ptr, (name, ra, ca)
            if not c_is_ptr:
                rt = ra.split(":")[1].strip()
                if "size_t" in ca:
                    assert rt == "usize", (name, ra, ca)
                elif "uint64_t" in ca:
                    assert rt == "u64", (name, ra, ca)
                elif re.search(r"\bunsigned\b", ca):
                    assert rt == "u32", (name, ra, ca)
                elif re.search(r"\bint\b", ca):
                    assert rt in ("c_int", "core::ffi::c_int"), (name, ra, ca)
    # KzgAmdConfig
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    end = hdr.index("} KzgAmdConfig;")
    c_fields = hdr[hdr.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    c_names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in c_fields.split(";") if d.strip()]
    src = open(rs).read()
    r_fields = re.search(r"#\[repr\(C\)\]\s*pub struct KzgAmdConfig \{(.*?)\}", src, flags=re.S).group(1)
    r_decl = [(m.group(1), m.group(2).strip()) for m in re.finditer(r"pub (\w+):\s*([^,]+),", r_fields)]
    assert [n for n, _ in r_decl] == c_names == ["struct_size", "device", "table_budget_bytes", "tuning"]
    assert [t for _, t in r_decl] == ["u32", "i32", "u64", "*const c_char"]
    # and the backend crate only calls what the sys crate offers
    sys_fns = set(re.findall(r"pub (?:unsafe )?fn (\w+)", src))
    for fn in ("g1.rs", "kzg_settings.rs", "fft_settings.rs"):
        used = set(re.findall(r"sys::(\w+)\(", open(os.path.join(ROOT, "rust-kzg_amd", "rust-backend", "src", fn)).read()))
        assert used <= sys_fns, (fn, used - sys_fns)


def test_configuration_parser_and_its_documented_table(tmp_path):
    """csrc/config.h on the host: the key table is well-formed, `kzgamd::Options::parse` / `resolve` accept what
    include/kzg_mi355x.h says they accept and refuse the rest (unknown key, missing / non-numeric value, out of range,
    a struct_size that is no version of KzgAmdConfig), the caller's struct beats the environment, and DESIGN.md §9
    lists exactly the keys of the table with their defaults and ranges."""
    import re
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "cfgcheck.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include "config.h"
using kzgamd::Options;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
int main() {
    const kzgamd::TuneKey* k = kzgamd::tune_keys();
    for (int i = 0; i < kzgamd::T_COUNT; ++i)
        printf("KEY %s %ld %ld %ld\n", k[i].name, k[i].dflt, k[i].lo, k[i].hi);
    std::string err;
    Options o;
    EXPECT(o.parse(nullptr, &err) && o.parse("", &err) && o.parse(" ; ,\n", &err));
    EXPECT(o.parse("spl=4;glv=0, window=13 fk20=-1\n", &err));
    EXPECT(o.t[kzgamd::T_SPL] == 4 && o.t[kzgamd::T_GLV] == 0 && o.t[kzgamd::T_WINDOW] == 13 && o.t[kzgamd::T_FK20] == -1);
    EXPECT(o.t[kzgamd::T_LEADERS] == 3);  // untouched keys keep their defaults
    EXPECT(!o.parse("sql=4", &err) && err.find("unknown key 'sql'") != std::string::npos);
    EXPECT(!o.parse("spl", &err) && err.find("no value") != std::string::npos);
    EXPECT(!o.parse("spl=", &err) && err.find("non-numeric") != std::string::npos);
    EXPECT(!o.parse("spl=x", &err) && err.find("non-numeric") != std::string::npos);
    EXPECT(!o.parse("spl=4x", &err));            // trailing garbage is a key without a value
    EXPECT(!o.parse("spl=17", &err) && err.find("out of range") != std::string::npos);
    EXPECT(!o.parse("glv=-1", &err) && !o.parse("combine_lanes=0", &err) && !o.parse("combine_lanes=5", &err));
    EXPECT(o.parse("g1_pair_max=1099511627776", &err));   // 2^40: the long range of the G1 stage keys
    // inside the range but not a value any engine honours: refused, not remapped
    EXPECT(!o.parse("spl=3", &err) && err.find("out of range") != std::string::npos);
    EXPECT(!o.parse("spl=5", &err) && !o.parse("blocksum_threads=100", &err) && !o.parse("fine_bits=6", &err));
    EXPECT(!o.parse("lgc=1", &err) && !o.parse("lgc=9", &err) && !o.parse("window=1", &err) && !o.parse("window_prepared=1", &err));
    EXPECT(!o.parse("sha_lanes=2", &err) && !o.parse("wide_fold_max=-1", &err) && !o.parse("tile_rows=8", &err));
    EXPECT(o.parse("spl=16;blocksum_threads=128;fine_bits=10;lgc=2;window=2;sha_lanes=1;sub_streams=0", &err));
    {   // the keys of the overlap forms that were removed (profiles/NOTES.md) are no keys any more
        Options x;
        EXPECT(!x.parse("groups=2", &err) && err.find("unknown key 'groups'") != std::string::npos);
        EXPECT(!x.parse("tail_pieces=2", &err) && err.find("unknown key 'tail_pieces'") != std::string::npos);
        EXPECT(!x.parse("sort_ahead=1", &err) && err.find("unknown key 'sort_ahead'") != std::string::npos);
    }
    // resolve: defaults < environment < struct
    setenv("KZGAMD_TUNING", "spl=2;lgc=8", 1);
    setenv("KZGAMD_FBW_MAX_GB", "24", 1);
    Options r;
    EXPECT(Options::resolve(r, nullptr, &err) && r.t[kzgamd::T_SPL] == 2 && r.t[kzgamd::T_LGC] == 8 && r.table_budget_gb == 24 && r.device == -1);
    KzgAmdConfig c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.device = 3;
    c.table_budget_bytes = 10000000000ull;
    c.tuning = "spl=8";
    EXPECT(Options::resolve(r, &c, &err) && r.t[kzgamd::T_SPL] == 8 && r.t[kzgamd::T_LGC] == 8 && r.table_budget_gb == 10 && r.device == 3);
    c.table_budget_bytes = KZGAMD_NO_TABLES;
    EXPECT(Options::resolve(r, &c, &err) && r.table_budget_gb == 0);
    c.table_budget_bytes = 0;  // 0 = not given: the environment's value stays
    EXPECT(Options::resolve(r, &c, &err) && r.table_budget_gb == 24);
    c.tuning = "nonsense=1";
    EXPECT(!Options::resolve(r, &c, &err));
    c.tuning = nullptr;
    c.struct_size = 8;
    EXPECT(!Options::resolve(r, &c, &err) && err.find("struct_size") != std::string::npos);
    c.struct_size = sizeof c + 16;  // a later, longer version of the struct: its known prefix is read
    EXPECT(Options::resolve(r, &c, &err));
    setenv("KZGAMD_TUNING", "spl=99", 1);  // a bad environment string fails the call as well
    EXPECT(!Options::resolve(r, nullptr, &err));
    printf("fails %d\n", fails);
    return fails != 0;
}
''')
    exe = tmp_path / "cfgcheck"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "fails 0" in res.stdout, res.stdout + res.stderr
    keys = [ln.split()[1:] for ln in res.stdout.splitlines() if ln.startswith("KEY ")]
    names = [k[0] for k in keys]
    assert len(names) == len(set(names)) == 46
    for name, d, lo, hi in keys:
        assert re.fullmatch(r"[a-z0-9_]+", name) and int(lo) <= int(d) <= int(hi), name
    # one row per key, same default and range
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec = design[design.index("## 9. Configuration and tuning keys"):]
    sec = sec[:sec.index("\n## 10.")]
    rows = re.findall(r"^\| `([a-z0-9_]+)` \| (-?\d+) \| (-?\d+) … (-?\d+) \|", sec, flags=re.M)
    assert [tuple(r) for r in rows] == [tuple(k) for k in keys]
    # and the header names the same four fields the parser reads
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for field in ("struct_size", "device", "table_budget_bytes", "tuning", "KZGAMD_NO_TABLES"):
        assert field in hdr


def test_take_key_extracts_the_keys_of_one_entry_point_as_the_three_scanners_did(tmp_path):
    """csrc/config.h, kzgamd::take_key: the extractor of the keys that belong to one entry point (pairing_gpu_min of
    kzgamd_kzg_new, fk20_table of kzgamd_fk20_new, mul_slice of the group multiplications).  The three scanners it
    replaced are kept in this program as the reference: on a table of strings — the key alone, first, last, in the
    middle and twice, every separator, the empty string, prefixes of other keys, malformed values, lo, hi and one beyond
    each — old and new give the same verdict, the same value and the same rest, and `Options::parse` makes the same of
    that rest.  The one difference is pinned: of two mul_slice tokens the old scanner tested both for a power of two,
    read_config tests the one that wins."""
    import shutil

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "takekey.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "config.h"
using kzgamd::Options;
using kzgamd::take_key;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// ---- the three scanners that kzg.hip, fk20.hip and groupmul.hip had before take_key, kept here as the reference
namespace old {
constexpr size_t SLICE_MIN = 64;
bool take_pairing_gpu_min(const char* str, long* value, std::string* rest) {
    static const char key[] = "pairing_gpu_min";
    auto is_sep = [](char c) { return c == ';' || c == ',' || c == ' ' || c == '\t' || c == '\n'; };
    const char* p = str;
    while (*p) {
        while (*p && is_sep(*p)) ++p;
        const char* e = p;
        while (*e && !is_sep(*e)) ++e;
        if (e == p) break;
        if ((size_t)(e - p) > sizeof key - 1 && !strncmp(p, key, sizeof key - 1) && p[sizeof key - 1] == '=') {
            char* end = nullptr;
            const long v = strtol(p + sizeof key, &end, 10);
            if (end != e || end == p + sizeof key || v < -1 || v > (1 << 20)) return false;
            *value = v;
        } else {
            if (!rest->empty()) *rest += ';';
            rest->append(p, e);
        }
        p = e;
    }
    return true;
}
bool take_fk20_table(const char* str, long* value, std::string* rest) {
    static const char key[] = "fk20_table";
    auto is_sep = [](char c) { return c == ';' || c == ',' || c == ' ' || c == '\t' || c == '\n'; };
    const char* p = str;
    while (*p) {
        while (*p && is_sep(*p)) ++p;
        const char* e = p;
        while (*e && !is_sep(*e)) ++e;
        if (e == p) break;
        if ((size_t)(e - p) > sizeof key - 1 && !strncmp(p, key, sizeof key - 1) && p[sizeof key - 1] == '=') {
            char* end = nullptr;
            const long v = strtol(p + sizeof key, &end, 10);
            if (end != e || end == p + sizeof key || v < -1 || v > 1) return false;
            *value = v;
        } else {
            if (!rest->empty()) *rest += ';';
            rest->append(p, e);
        }
        p = e;
    }
    return true;
}
bool take_mul_slice(const char* str, size_t* value) {
    static const char key[] = "mul_slice";
    auto is_sep = [](char c) { return c == ';' || c == ',' || c == ' ' || c == '\t' || c == '\n'; };
    const char* p = str;
    while (*p) {
        while (*p && is_sep(*p)) ++p;
        const char* e = p;
        while (*e && !is_sep(*e)) ++e;
        if (e == p) break;
        if ((size_t)(e - p) <= sizeof key - 1 || strncmp(p, key, sizeof key - 1) || p[sizeof key - 1] != '=') return false;
        char* end = nullptr;
        const long long v = strtoll(p + sizeof key, &end, 10);
        if (end != e || end == p + sizeof key || v < (long long)SLICE_MIN || v > (1ll << 30) || (v & (v - 1))) return false;
        *value = (size_t)v;
        p = e;
    }
    return true;
}
}  // namespace old

// what groupmul.hip's read_config makes of take_key: the one key of its calls, a power of two from SLICE_MIN
static bool new_mul_slice(const char* str, size_t* value) {
    long long v = 1 << 18;  // SLICE_DEFAULT: what stays when the key is not there
    std::string rest;
    if (!take_key(str, "mul_slice", (long long)old::SLICE_MIN, 1ll << 30, &v, &rest) || !rest.empty() || (v & (v - 1))) return false;
    *value = (size_t)v;
    return true;
}
static bool parses(const std::string& s) {
    Options o;
    std::string err;
    return o.parse(s.c_str(), &err);
}
struct Got {
    bool ok;
    long long v;
    std::string rest;
};
static Got take(const char* s, const char* key, long long lo, long long hi) {
    Got g{false, -77, ""};
    g.ok = take_key(s, key, lo, hi, &g.v, &g.rest);
    return g;
}

int main() {
    std::vector<std::string> table = {
        // the strings whose verdicts the entry points must keep
        "mul_slices=64", "mul_slice=", "mul_slice=96", "mul_slice=64;spl=1", "fk20_table=", "fk20_table=2", "fk20_table=0;nonsense=1",
        "combine=0;fk20_table=0,g1_wide_max=4096",
        // the empty string, separators alone
        "", ";", " ; ,\t\n",
        // prefixes of other keys, keys without a value, text after the number
        "fk20_tables=1", "fk20_table", "fk20_table=1x", "fk20_table=x", "fk20_table=-", "fk20_table==1", "xfk20_table=1", "pairing_gpu_min", "pairing_gpu_mins=3",
        "pairing_gpu_min=4x", "mul_slice", "mul_slice=64x", "mul_slice=0x40", "fk20_table= 1", "fk20_table=+1", "fk20_table=01",
        // numbers no long holds
        "pairing_gpu_min=99999999999999999999999", "mul_slice=99999999999999999999999", "fk20_table=-99999999999999999999999"};
    // each key alone, first, last, in the middle, twice (the last one wins), with every separator
    const char* seps[] = {";", ",", " ", "\t", "\n", ";;", " ; "};
    struct K { const char* key; std::vector<const char*> vals; };
    const K keys[] = {
        {"pairing_gpu_min", {"-2", "-1", "0", "4", "1048576", "1048577"}},      // lo - 1, lo, ..., hi, hi + 1
        {"fk20_table", {"-2", "-1", "0", "1", "2"}},
        {"mul_slice", {"32", "63", "64", "65", "128", "262144", "1073741824", "1073741825", "2147483648"}},
    };
    for (const K& k : keys)
        for (const char* v : k.vals) {
            const std::string kv = std::string(k.key) + "=" + v;
            table.push_back(kv);
            for (const char* sep : seps) {
                table.push_back(kv + sep + "spl=4");
                table.push_back("spl=4" + std::string(sep) + kv);
                table.push_back("glv=0" + std::string(sep) + kv + sep + "spl=4");
                table.push_back(kv + sep);
                table.push_back(sep + kv);
                table.push_back(kv + sep + k.key + "=" + k.vals[2]);
                table.push_back(std::string(k.key) + "=" + k.vals[2] + sep + kv);
                table.push_back(kv + sep + "nonsense=1");
                table.push_back(kv + sep + "spl=3");
            }
        }
    size_t last_wins = 0;
    // old and new agree on every string of the table: verdict, value and the rest handed to Options::parse
    for (const std::string& s : table) {
        long ov = -77;
        std::string orest;
        bool ook = old::take_pairing_gpu_min(s.c_str(), &ov, &orest);
        Got g = take(s.c_str(), "pairing_gpu_min", -1, 1 << 20);
        if (ook != g.ok || (ook && (ov != g.v || orest != g.rest || parses(orest) != parses(g.rest)))) {
            printf("pairing_gpu_min differs on '%s'\n", s.c_str());
            ++fails;
        }
        ov = -77;
        orest.clear();
        ook = old::take_fk20_table(s.c_str(), &ov, &orest);
        g = take(s.c_str(), "fk20_table", -1, 1);
        if (ook != g.ok || (ook && (ov != g.v || orest != g.rest || parses(orest) != parses(g.rest)))) {
            printf("fk20_table differs on '%s'\n", s.c_str());
            ++fails;
        }
        size_t os = 12345, ns = 12345;
        ook = old::take_mul_slice(s.c_str(), &os);
        const bool nok = new_mul_slice(s.c_str(), &ns);
        if (ook && os == 12345) os = 1 << 18;  // the old scanner left the caller's default alone
        // The one difference, pinned: the old scanner tested "a power of two" on every mul_slice token, read_config
        // tests it on the value take_key hands back, the last one.  "mul_slice=65;mul_slice=64" was refused and is
        // now a slice of 64 (65 is inside the range; a first value outside it is refused by both).
        const size_t first = s.find("mul_slice=65"), last = s.rfind("mul_slice=");
        if (!ook && nok && first != std::string::npos && last > first) {
            EXPECT(ns == 64);
            ++last_wins;
            continue;
        }
        if (ook != nok || (ook && os != ns)) {
            printf("mul_slice differs on '%s'\n", s.c_str());
            ++fails;
        }
    }
    printf("table %zu\n", table.size());
    EXPECT(last_wins == sizeof seps / sizeof seps[0]);
    // the verdicts themselves
    size_t sl = 1;
    EXPECT(!new_mul_slice("mul_slices=64", &sl) && !new_mul_slice("mul_slice=", &sl) && !new_mul_slice("mul_slice=96", &sl));
    EXPECT(!new_mul_slice("mul_slice=64;spl=1", &sl) && !new_mul_slice("mul_slice=32", &sl) && !new_mul_slice("mul_slice=2147483648", &sl) && sl == 1);
    EXPECT(new_mul_slice("", &sl) && sl == (1u << 18) && new_mul_slice("mul_slice=64", &sl) && sl == 64);
    EXPECT(new_mul_slice(" mul_slice=128\n", &sl) && sl == 128 && new_mul_slice("mul_slice=64,mul_slice=1073741824", &sl) && sl == (1u << 30));
    EXPECT(!take("fk20_table=", "fk20_table", -1, 1).ok && !take("fk20_table=2", "fk20_table", -1, 1).ok);
    EXPECT(!take("fk20_table=-2", "fk20_table", -1, 1).ok && !take("spl=4;fk20_table=1x", "fk20_table", -1, 1).ok);
    Got g = take("fk20_table=0;nonsense=1", "fk20_table", -1, 1);
    EXPECT(g.ok && g.v == 0 && g.rest == "nonsense=1" && !parses(g.rest));
    g = take("combine=0;fk20_table=0,g1_wide_max=4096", "fk20_table", -1, 1);
    EXPECT(g.ok && g.v == 0 && g.rest == "combine=0;g1_wide_max=4096" && parses(g.rest));
    {
        Options o;
        std::string err;
        EXPECT(o.parse(g.rest.c_str(), &err) && o.t[kzgamd::T_COMBINE] == 0 && o.t[kzgamd::T_G1_WIDE_MAX] == 4096);
    }
    g = take("", "fk20_table", -1, 1);
    EXPECT(g.ok && g.v == -77 && g.rest.empty());  // no key: the caller's default stays
    g = take("fk20_tables=1 fk20_table\tfk20_tabl=1", "fk20_table", -1, 1);
    EXPECT(g.ok && g.v == -77 && g.rest == "fk20_tables=1;fk20_table;fk20_tabl=1" && !parses(g.rest));
    g = take("fk20_table=1", "fk20_table", -1, 1);
    EXPECT(g.ok && g.v == 1 && g.rest.empty());
    g = take("fk20_table=-1;spl=4", "fk20_table", -1, 1);
    EXPECT(g.ok && g.v == -1 && g.rest == "spl=4");
    g = take("spl=4,glv=0 window=13\tfk20=-1\npairing_gpu_min=1048576", "pairing_gpu_min", -1, 1 << 20);
    EXPECT(g.ok && g.v == (1 << 20) && g.rest == "spl=4;glv=0;window=13;fk20=-1" && parses(g.rest));
    g = take("pairing_gpu_min=0;spl=4;pairing_gpu_min=9", "pairing_gpu_min", -1, 1 << 20);
    EXPECT(g.ok && g.v == 9 && g.rest == "spl=4");  // the last one wins
    EXPECT(!take("pairing_gpu_min=1048577", "pairing_gpu_min", -1, 1 << 20).ok && !take("pairing_gpu_min=-2", "pairing_gpu_min", -1, 1 << 20).ok);
    EXPECT(take("pairing_gpu_min=-1", "pairing_gpu_min", -1, 1 << 20).v == -1);
    printf("fails %d\n", fails);
    return fails != 0;
}
''')
    exe = tmp_path / "takekey"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "fails 0" in res.stdout, res.stdout + res.stderr
    assert int(re.search(r"^table (\d+)$", res.stdout, flags=re.M).group(1)) > 1000
    # the three keys stay out of the library's table of keys and of the rows DESIGN.md §9 generates from it
    cfg = open(os.path.join(ROOT, "rust-kzg_amd", "csrc", "config.h")).read()
    table = cfg[cfg.index("inline const TuneKey* tune_keys()"):cfg.index("inline bool tune_value_allowed")]
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec = design[design.index("## 9. Configuration and tuning keys"):]
    sec = sec[:sec.index("\n## 10.")]
    rows = re.findall(r"^\| `([a-z0-9_]+)` \| (-?\d+) \| (-?\d+) … (-?\d+) \|", sec, flags=re.M)  # the rows of the library's table
    for key in ("pairing_gpu_min", "fk20_table", "mul_slice"):
        assert '{"%s"' % key not in table and key not in [r[0] for r in rows]


def test_host_call_frame_maps_errors_and_releases_the_handle(tmp_path):
    """csrc/host_call.h without a device (the HIP calls it makes are this program's own, counted): the status of a
    body that returns one, of a void body, of DevErr{hipErrorOutOfMemory} (-102), of the MSM engine's
    DevErr{hipErrorInvalidValue, text} (-101), of std::bad_alloc and of an int (-2); DEV_TRY throws the code with the
    expression's text; run_call runs the body on the handle's device with its lock held,
    synchronises once on either way out and leaves the lock free after every throwing body; DevBuf grows and drops,
    ScopedBuf frees; create_handle gives dev_code or -4 and deletes what did not make it.  DevArray, the one owner of
    device memory: typed growth in elements, freed at scope exit and once only after drop(), moves, a failed hipMalloc
    (ensure throws the code and leaves the array empty), a group released as a whole before any of it is allocated
    (drop_all), and a creation whose init throws after ensure — nothing leaks, with no destructor naming a buffer.  Built
    with the address and undefined-behaviour sanitizers as a plain executable."""
    import shutil

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = tmp_path / "hostcall.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include "host_call.h"
// the HIP runtime of this program: every call succeeds and is counted, no device anywhere; hipMalloc and hipFree are
// logged in order ('M' / 'F'), and the fail_at-th hipMalloc from now (1 = the next) fails with hipErrorOutOfMemory
static int syncs = 0, frees = 0, mallocs = 0, device = 0, fail_at = 0;
static size_t last_bytes = 0;
static std::string order;
extern "C" {
hipError_t hipGetDevice(int* d) { *d = device; return hipSuccess; }
hipError_t hipSetDevice(int d) { device = d; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { ++syncs; return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) {
    if (fail_at > 0 && --fail_at == 0) { order += 'X'; return hipErrorOutOfMemory; }
    ++mallocs; order += 'M'; last_bytes = n; *p = ::operator new(n); return hipSuccess;
}
hipError_t hipFree(void* p) { ++frees; order += 'F'; ::operator delete(p); return hipSuccess; }
}
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Handle {
    std::mutex mu;
    int device = 3;
    hipStream_t st = nullptr;
    kzgamd::DevBuf buf;
    bool made = false;
    static int live;
    Handle() { ++live; }
    ~Handle() { --live; }  // the buffer frees itself
};
int Handle::live = 0;
// the handle's lock is free again: a second call would not block
static bool unlocked(Handle& h) {
    if (!h.mu.try_lock()) return false;
    h.mu.unlock();
    return true;
}
int main() {
    using namespace kzgamd;
    EXPECT(dev_code(hipErrorOutOfMemory) == -102 && dev_code(hipErrorUnknown) == -1099);
    // the pure mapping
    EXPECT(status_of([] { return 7; }) == 7);
    EXPECT(status_of([] {}) == 0);
    EXPECT(status_of([] { DEV_TRY(hipErrorOutOfMemory); }) == -102);
    EXPECT(status_of([]() -> int { throw std::bad_alloc(); }) == -2);
    EXPECT(status_of([] { throw DevErr{hipErrorInvalidValue, "npoints exceeds the prepared size"}; }) == -101);  // the engine's own
    EXPECT(status_of([] { throw 5; }) == -2);
    try {
        DEV_TRY(hipErrorOutOfMemory);
        EXPECT(false);
    } catch (const DevErr& e) {
        EXPECT(e.e == hipErrorOutOfMemory && !strcmp(e.what, "hipErrorOutOfMemory"));
    }
    EXPECT(!strcmp(DevErr{hipErrorOutOfMemory}.what, ""));  // the code alone still makes one
    // the frame of a call: one synchronisation when the body returns, one more before unwinding when it throws
    Handle h;
    int seen_device = -1;
    syncs = 0;
    EXPECT(run_call(&h, [&] { seen_device = device; return 7; }) == 7 && syncs == 1 && unlocked(h));
    EXPECT(seen_device == 3 && device == 0);  // the body ran on the handle's device, the caller's is back
    syncs = 0;
    EXPECT(run_call(&h, [&] { EXPECT(!h.mu.try_lock()); }) == 0 && syncs == 1 && unlocked(h));
    syncs = 0;
    EXPECT(run_call(&h, [] { throw DevErr{hipErrorOutOfMemory}; }) == -102 && syncs == 1 && unlocked(h));
    syncs = 0;
    EXPECT(run_call(&h, []() -> int { throw std::bad_alloc(); }) == -2 && syncs == 1 && unlocked(h));
    syncs = 0;
    EXPECT(run_call(&h, [] { throw DevErr{hipErrorInvalidValue, "npoints exceeds the prepared size"}; }) == -101 && syncs == 1 && unlocked(h));
    syncs = 0;
    EXPECT(run_call(&h, [] { throw 5; }) == -2 && syncs == 1 && unlocked(h));
    EXPECT(run_call(&h, [] { return 0; }) == 0 && device == 0);
    // buffers
    {
        DevBuf b;
        b.ensure(100);
        void* first = b.p;
        b.ensure(50);
        EXPECT(b.p == first && b.cap == 100 && mallocs == 1 && frees == 0);
        b.ensure(200);
        EXPECT(b.cap == 200 && mallocs == 2 && frees == 1);
        b.drop();
        EXPECT(!b.p && b.cap == 0 && frees == 2);
        ScopedBuf s;
        s.alloc(0);
        EXPECT(s.p && mallocs == 3);
    }
    EXPECT(frees == 3);
    // DevArray: typed growth, counted in elements
    {
        DevArray<uint32_t> a;
        a.ensure(100);
        uint32_t* first = a.p;
        EXPECT(a.cap == 100 && last_bytes == 400 && mallocs == 4 && frees == 3);
        a.ensure(50);
        EXPECT(a.p == first && a.cap == 100 && mallocs == 4 && frees == 3);
        order.clear();
        a.ensure(200);
        EXPECT(a.cap == 200 && last_bytes == 800 && mallocs == 5 && frees == 4 && order == "FM");
        EXPECT(a.as<unsigned char>() == (unsigned char*)a.p);
    }
    EXPECT(frees == 5 && mallocs == 5);  // leaving the scope frees without drop()
    {
        DevArray<uint32_t> a;
        a.ensure(4);
        a.drop();
        EXPECT(!a.p && a.cap == 0 && frees == 6);
        a.drop();  // idempotent
        EXPECT(frees == 6);
    }
    EXPECT(frees == 6 && mallocs == 6);  // drop() then the destructor: freed once
    // moves
    {
        DevArray<uint32_t> a;
        a.ensure(8);
        uint32_t* block = a.p;
        DevArray<uint32_t> b(std::move(a));
        EXPECT(!a.p && a.cap == 0 && b.p == block && b.cap == 8 && frees == 6);
        DevArray<uint32_t> c;
        c.ensure(16);
        EXPECT(mallocs == 8);
        c = std::move(b);  // onto a full buffer: its old block goes
        EXPECT(frees == 7 && c.p == block && c.cap == 8 && !b.p && b.cap == 0);
    }
    EXPECT(frees == 8 && mallocs == 8);  // the pair freed once in total
    static_assert(!std::is_copy_constructible_v<DevArray<int>> && !std::is_copy_assignable_v<DevArray<int>>, "move-only");
    // a failed hipMalloc
    {
        DevArray<uint32_t> a;
        fail_at = 1;
        EXPECT(status_of([&] { a.ensure(10); }) == -102 && a.p == nullptr && a.cap == 0);
        a.ensure(10);
        order.clear();
        fail_at = 1;
        EXPECT(status_of([&] { a.ensure(20); }) == -102 && a.p == nullptr && a.cap == 0 && order == "FX");  // the old block went first
        fail_at = 1;
        EXPECT(status_of([&] { a.ensure(20); }) == -102 && a.p == nullptr && a.cap == 0);
    }
    EXPECT(frees == 9 && mallocs == 9 && fail_at == 0);
    // a group: released as a whole before any of it is allocated
    {
        DevArray<uint32_t> a;
        DevArray<unsigned char> b;
        auto grow = [&](size_t n) {
            return status_of([&] {
                drop_all(a, b);
                a.ensure(n);
                b.ensure(n);
            });
        };
        EXPECT(grow(4) == 0);
        order.clear();
        EXPECT(grow(8) == 0 && order == "FFMM");
        order.clear();
        fail_at = 2;
        EXPECT(grow(16) == -102 && order == "FFMX");
        EXPECT(a.p && a.cap == 16 && !b.p && b.cap == 0);  // the first block is still owned ...
    }
    EXPECT(mallocs == 14 && frees == 14);  // ... and freed once at scope exit
    EXPECT(blocks(0) == 0 && blocks(1) == 1 && blocks(256) == 1 && blocks(257) == 2 && blocks(65, 64) == 2);
    EXPECT(next_pow2(0) == 1 && next_pow2(1) == 1 && next_pow2(3) == 4 && next_pow2(4096) == 4096 && next_pow2(4097) == 8192);
    // the frame of a creation
    int err = 0;
    Handle* made = create_handle<Handle>(5, &err, [&](Handle* c) { c->made = device == 5 && c->device == 5; c->buf.ensure(8); });
    EXPECT(made && made->made && err == 0 && device == 0 && Handle::live == 2);
    delete made;
    err = 0;
    EXPECT(!create_handle<Handle>(5, &err, [](Handle* c) { c->buf.ensure(8); DEV_TRY(hipErrorOutOfMemory); }) && err == -102);
    err = 0;
    EXPECT(!create_handle<Handle>(5, &err, [](Handle*) { throw std::bad_alloc(); }) && err == -4);
    EXPECT(Handle::live == 1 && device == 0 && mallocs == frees);  // what did not make it was deleted
    order.clear();
    err = 0;
    EXPECT(!create_handle<Handle>(5, &err, [](Handle* c) { c->buf.ensure(8); throw std::bad_alloc(); }) && err == -4);
    EXPECT(order == "MF" && mallocs == frees && Handle::live == 1);  // ~Handle names no buffer: the member freed itself
    printf("fails %d\n", fails);
    return fails != 0;
}
''')
    exe = tmp_path / "hostcall"
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"),
                           "-I", os.path.join(rocm, "include"), str(src), "-o", str(exe), "-lpthread"])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "fails 0" in res.stdout, res.stdout + res.stderr


@pytest.mark.parametrize("portable", [False, True])
def test_host_sha256_both_code_paths_against_hashlib(tmp_path, portable):
    """csrc/sha256.h hashes the Fiat-Shamir transcripts of host-buffer calls (kzg/src/eip_4844.rs:236-238, :920-945): its
    SHA-NI path is the one the GPU box's host runs, its portable path the one nothing else here would ever run — both
    against hashlib on every padding boundary and on transcript-sized messages fed in ragged pieces."""
    import hashlib
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    lengths = list(range(0, 130)) + [191, 192, 193, 4095, 4096, 16 + 131072 + 48, 16 + 8 + 8 + 64 * 144 + 7]
    src = tmp_path / "shacheck.cpp"
    src.write_text(("#define __builtin_cpu_supports(x) 0\n" if portable else "") + r'''
#include <cstdio>
#include <vector>
#include "sha256.h"
static uint64_t st = 88172645463325252ull;
static uint32_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 11); }
int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        const size_t n = strtoul(argv[a], nullptr, 10);
        std::vector<uint8_t> m(n + 1);
        for (size_t i = 0; i < n; ++i) m[i] = (uint8_t)(i * 131 + n);
        kzgamd::Sha256 h;
        size_t off = 0;
        while (off < n) {  // ragged pieces: 1 .. 200 bytes
            size_t take = 1 + rnd() % 200;
            if (take > n - off) take = n - off;
            h.update(m.data() + off, take);
            off += take;
        }
        uint8_t d[32];
        h.finish(d);
        for (int i = 0; i < 32; ++i) printf("%02x", d[i]);
        printf("\n");
        h.reset();  // a reused object starts clean
        h.update(m.data(), n);
        uint8_t d2[32];
        h.finish(d2);
        if (memcmp(d, d2, 32)) printf("reuse differs at %zu\n", n);
    }
    return 0;
}
''')
    exe = tmp_path / "shacheck"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)] + [str(n) for n in lengths]).decode().split("\n")
    out = [ln for ln in out if ln]
    assert len(out) == len(lengths), out[-3:]
    for n, got in zip(lengths, out):
        msg = bytes((i * 131 + n) & 0xFF for i in range(n))
        assert got == hashlib.sha256(msg).hexdigest(), n


def _g1_encodings(L, O, rnd):
    """compressed G1 encodings for the (de)serialisation tests: infinity, points of G1, curve points outside G1 (both
    signs), then every class of invalid encoding; returns (encodings, number of valid ones)"""
    g = O.G1()
    L.og1_generator(C.byref(g))

    def comp(p):
        buf = C.create_string_buffer(48)
        L.og1_compress(buf, C.byref(p))
        return buf.raw

    enc = [comp(O.G1())]  # infinity: c0 00 ... 00
    for k in [1, 2, 3, O.R - 1] + [rnd.randrange(1, O.R) for _ in range(24)]:
        p = O.G1()
        kf = O.fr_from_int(k)
        L.og1_mul(C.byref(p), C.byref(g), C.byref(kf))
        enc.append(comp(p))
    # on the curve, outside G1: small x with a square x^3 + 4, both signs of y
    x = 0
    outside = 0
    while outside < 6:
        x += 1
        rhs = (pow(x, 3, O.P) + 4) % O.P
        y = pow(rhs, (O.P + 1) // 4, O.P)
        if y * y % O.P == rhs:
            for sign in (0, 0x20):
                enc.append(bytes([0x80 | sign | (x >> 376)]) + (x & ((1 << 376) - 1)).to_bytes(47, "big"))
            outside += 1
    good = enc[5]
    bad = [
        bytes([good[0] & 0x7F]) + good[1:],                 # compression flag missing
        bytes([0xC0]) + bytes(46) + b"\x01",                # infinity with a non-zero x
        bytes([0xE0]) + bytes(47),                          # infinity with the sign flag
        bytes([0x80 | (O.P >> 376)]) + (O.P & ((1 << 376) - 1)).to_bytes(47, "big"),  # x = p
        bytes([0x9F]) + b"\xff" * 47,                       # x >= p
    ]
    x = 0
    while len(bad) < 8:                                     # x^3 + 4 not a square: not on the curve
        x += 1
        rhs = (pow(x, 3, O.P) + 4) % O.P
        if pow(rhs, (O.P - 1) // 2, O.P) != 1:
            bad.append(bytes([0x80]) + x.to_bytes(47, "big"))
    # tests/g1_encodings.py on top: low-order and torsion points, every flag combination, the range edges
    import g1_encodings

    cat = g1_encodings.catalogue()
    enc += [b for _, b, cls in cat if cls != 1]
    valid = len(enc)
    enc += bad + [b for _, b, cls in cat if cls == 1]
    return enc, valid


def build_g1check(tmp_path):
    """the stand-alone program over csrc/host_g1.h: per line of compressed hex on stdin `bad` or `ok <in G1> <compressed
    again>`, then the doublings and sums of the decoded points through the batch compression"""
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "g1check.cpp"
    src.write_text(r'''
#include <cstdio>
#include <vector>
#include "host_g1.h"
using namespace kzgamd;
static void hex(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; ++i) printf("%02x", p[i]); }
int main() {
    char line[256];
    std::vector<blst_p1> pts;
    while (fgets(line, sizeof line, stdin)) {
        uint8_t in[48];
        for (int i = 0; i < 48; ++i) { unsigned v; sscanf(line + 2 * i, "%2x", &v); in[i] = (uint8_t)v; }
        blst_p1 p;
        if (!host_p1_uncompress(&p, in)) { printf("bad\n"); continue; }
        uint8_t c[48];
        host_p1_compress(c, &p);
        printf("ok %d ", host_p1_in_g1(&p) ? 1 : 0);
        hex(c, 48);
        printf("\n");
        pts.push_back(p);
    }
    // doublings, sums (P + P, P + (-P), P + infinity among them) through the batch compression
    std::vector<blst_p1> out;
    auto J = [](const blst_p1& p) { const ff::Fp* P = reinterpret_cast<const ff::Fp*>(&p); return HostJac{P[0], P[1], P[2]}; };
    auto put = [&](const HostJac& j) { blst_p1 p; ff::Fp* P = reinterpret_cast<ff::Fp*>(&p); P[0] = j.x; P[1] = j.y; P[2] = j.z; out.push_back(p); };
    for (size_t i = 0; i < pts.size(); ++i) {
        const HostJac a = J(pts[i]), b = J(pts[(i + 1) % pts.size()]);
        HostJac d = host_jac_dbl(a);
        put(d);                       // 2a (non-trivial Z from here on)
        put(host_jac_add(d, b));      // 2a + b
        put(host_jac_add(a, a));      // the doubling branch of the addition
        HostJac n = d;
        n.y = hfp::neg(n.y);
        put(host_jac_add(d, n));      // infinity
        put(host_jac_mul_u64(a, 0xd201000000010000ull + i));
    }
    std::vector<uint8_t> c(out.size() * 48);
    host_p1_compress_batch(c.data(), out.data(), out.size());
    for (size_t i = 0; i < out.size(); ++i) { printf("c "); hex(c.data() + 48 * i, 48); printf("\n"); }
    return 0;
}
''')
    exe = tmp_path / "g1check"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def test_host_g1_serialisation_and_subgroup_test_against_the_oracle(tmp_path, oracle):
    """csrc/host_g1.h (the host side of bytes_to_kzg_commitment, compute_challenge's commitment, commitment checks of
    small proof batches, the Horner tail of variable-base host calls): uncompress / compress / batch compress, the
    Jacobian doubling and addition with their exceptional cases, and the endomorphism subgroup test, against the oracle
    on points of G1, curve points outside G1 and every class of invalid encoding (FsG1::from_bytes,
    blst/src/types/g1.rs:65-87)."""
    import random
    import shutil
    import subprocess

    import oracle_ffi as O

    L = oracle.lib()
    rnd = random.Random(404)
    g = O.G1()
    L.og1_generator(C.byref(g))

    def comp(p):
        buf = C.create_string_buffer(48)
        L.og1_compress(buf, C.byref(p))
        return buf.raw

    enc, valid = _g1_encodings(L, O, rnd)

    exe = build_g1check(tmp_path)
    out = subprocess.run([str(exe)], input="\n".join(e.hex() for e in enc) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    heads, sums = [ln for ln in out if ln and not ln.startswith("c ")], [ln[2:] for ln in out if ln.startswith("c ")]
    assert len(heads) == len(enc)
    pts = []
    for i, (e, ln) in enumerate(zip(enc, heads)):
        a = O.G1Affine()
        ok = L.og1_uncompress(C.byref(a), e)
        assert (ln != "bad") == bool(ok) == (i < valid), (i, e.hex(), ln)
        if not ok:
            continue
        p = O.G1()
        L.og1_from_affine(C.byref(p), C.byref(a))
        if e[0] & 0x40:
            p = O.G1()
        _, in_g1, again = ln.split()
        assert int(in_g1) == L.og1_in_subgroup(C.byref(p)), (i, e.hex())
        assert again == e.hex() == comp(p).hex(), i
        pts.append(p)
    import g1_encodings

    # the six outside points, both signs, and the catalogue's
    assert sum(1 for ln in heads if ln.startswith("ok 0")) == 12 + len(g1_encodings.by_class(2))
    assert len(sums) == 5 * len(pts)
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        d, s, n, m = O.G1(), O.G1(), O.G1(), O.G1()
        L.og1_dbl(C.byref(d), C.byref(a))
        L.og1_add_or_dbl(C.byref(s), C.byref(d), C.byref(b))
        kf = O.fr_from_int(0xd201000000010000 + i)
        L.og1_mul(C.byref(m), C.byref(a), C.byref(kf))
        want = [comp(d).hex(), comp(s).hex(), comp(d).hex(), comp(O.G1()).hex(), comp(m).hex()]
        assert sums[5 * i:5 * i + 5] == want, i


def test_host_p1_to_affine_and_its_batch_against_the_oracle(tmp_path, oracle):
    """csrc/host_g1.h, host_p1_to_affine and host_p1_to_affine_batch (the setup points of kzgamd_kzg_new, the table
    points of kzgamd_fk20_new and of the EIP-7594 cell proofs, the base of kzgamd_g1_mul_batch): n = 0, 1 (the identity,
    a point), 2, and 65 with the identity first, last, in the middle, in every slot in turn and everywhere; points with
    Z = 1 and with Z != 1; the same points through a strided, reversed `point_at`.  The batch is bit-equal to the
    single-point function (checked in the program), and both to the oracle's affine coordinates; the identity is (0, 0)
    in the batch and leaves x, y alone in the single form."""
    import random
    import shutil

    import oracle_ffi as O

    L = oracle.lib()
    rnd = random.Random(1729)
    g = O.G1()
    L.og1_generator(C.byref(g))
    pool = [O.G1()]  # index 0: the identity (Z == 0)
    for i in range(65):
        p, kf = O.G1(), O.fr_from_int(rnd.randrange(1, O.R))
        L.og1_mul(C.byref(p), C.byref(g), C.byref(kf))
        if i % 8 == 0:  # Z = 1
            a = O.G1Affine()
            L.og1_to_affine(C.byref(a), C.byref(p))
            p = O.G1()
            L.og1_from_affine(C.byref(p), C.byref(a))
        elif i % 8 == 1:  # another Z of the same point
            d = O.G1()
            L.og1_add_or_dbl(C.byref(d), C.byref(p), C.byref(g))
            p = d
        pool.append(p)
    one = bytes(g.z)
    assert sum(1 for p in pool[1:] if bytes(p.z) == one) >= 8 and sum(1 for p in pool[1:] if bytes(p.z) != one) >= 40
    full = list(range(1, 66))
    cases = [[], [0], [5], [1, 2], [0, 3], [3, 0], [0, 0], full, [0] * 65]
    for slot in range(65):  # the identity in every slot in turn: first, middle and last among them
        cases.append(full[:slot] + [0] + full[slot + 1:])
    cases.append([0] + full[1:32] + [0] + full[33:64] + [0])
    text = "".join("pt %s\n" % bytes(p).hex() for p in pool) + "".join("case %s\n" % " ".join(map(str, c)) for c in cases)

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "affine.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "host_g1.h"
using namespace kzgamd;
static void hex(const void* p, size_t n) { for (size_t i = 0; i < n; ++i) printf("%02x", ((const uint8_t*)p)[i]); }
int main() {
    std::vector<blst_p1> pool;
    std::string line;
    int c, bad = 0;
    while (true) {
        line.clear();
        while ((c = getchar()) != EOF && c != '\n') line.push_back((char)c);
        if (line.empty() && c == EOF) break;
        if (line.rfind("pt ", 0) == 0) {  // a Jacobian point, the bytes of a blst_p1
            blst_p1 p;
            for (size_t i = 0; i < sizeof p; ++i) { unsigned v; sscanf(line.c_str() + 3 + 2 * i, "%2x", &v); ((uint8_t*)&p)[i] = (uint8_t)v; }
            ff::Fp xy[2];
            memset(xy, 0xa5, sizeof xy);
            const ff::Fp before = xy[0];
            const bool inf = host_p1_to_affine(&p, xy[0], xy[1]);
            if (inf && (xy[0] != before || xy[1] != before)) ++bad;  // the identity leaves x and y alone
            printf("one %d ", inf ? 1 : 0);
            hex(xy, sizeof xy);
            printf("\n");
            pool.push_back(p);
        } else if (line.rfind("case", 0) == 0) {  // indices into the pool
            std::vector<blst_p1> pts;
            char* q = &line[4];
            while (*q) {
                char* e;
                const long v = strtol(q, &e, 10);
                if (e == q) break;
                pts.push_back(pool[(size_t)v]);
                q = e;
            }
            const size_t n = pts.size();
            std::vector<ff::Fp> aff(2 * n + 1), strided(2 * n + 1);
            memset(aff.data(), 0x5a, aff.size() * sizeof(ff::Fp));
            memset(strided.data(), 0x5a, strided.size() * sizeof(ff::Fp));
            const ff::Fp guard = aff[2 * n];
            host_p1_to_affine_batch(aff.data(), n, [&](size_t i) { return &pts[i]; });
            // the same points at every third slot of a longer array, in reverse order
            std::vector<blst_p1> wide(3 * n + 1);
            memset(wide.data(), 0x33, wide.size() * sizeof(blst_p1));
            for (size_t i = 0; i < n; ++i) wide[3 * (n - 1 - i) + 1] = pts[i];
            host_p1_to_affine_batch(strided.data(), n, [&](size_t i) { return &wide[3 * (n - 1 - i) + 1]; });
            if (memcmp(aff.data(), strided.data(), aff.size() * sizeof(ff::Fp)) || aff[2 * n] != guard) ++bad;  // nothing past 2n written
            for (size_t i = 0; i < n; ++i) {  // bit-equal to the single-point function
                ff::Fp x = ff::Fp::zero(), y = ff::Fp::zero();
                host_p1_to_affine(&pts[i], x, y);
                if (x != aff[2 * i] || y != aff[2 * i + 1]) ++bad;
            }
            printf("aff ");
            hex(aff.data(), 2 * n * sizeof(ff::Fp));
            printf("\n");
        }
    }
    printf("bad %d\n", bad);
    return bad != 0;
}
''')
    exe = tmp_path / "affine"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and "bad 0" in res.stdout, res.stdout[-2000:] + res.stderr
    out = res.stdout.split("\n")
    ones, affs = [ln.split() for ln in out if ln.startswith("one ")], [ln[4:] for ln in out if ln.startswith("aff ")]
    assert len(ones) == len(pool) and len(affs) == len(cases)
    want = []
    for i, p in enumerate(pool):
        if i == 0:
            want.append(bytes(96).hex())
            assert ones[i][1] == "1" and ones[i][2] == "a5" * 96
            continue
        a = O.G1Affine()
        L.og1_to_affine(C.byref(a), C.byref(p))
        assert L.og1_affine_on_curve(C.byref(a))
        want.append(bytes(a).hex())
        assert ones[i][1] == "0" and ones[i][2] == want[i], i
    for c, got in zip(cases, affs):
        assert got == "".join(want[i] for i in c), c


def test_glv_split_identity_and_bounds_on_the_host(tmp_path):
    """kzgamd::glv_split (glv.hip.h; the same function runs in the MSM's digit kernels and, on the host, for the roots
    of fft_g1): k = s1*k1 + s2*k2*x^2 (mod r) with both halves below 2^126.5 — what lets ceil(128/c) signed windows never
    carry out of the top one — on the boundaries of every branch-free select (0, 1, (r-1)/2 and its neighbours, r - 1,
    multiples of x^2 and of x^2/2 and their neighbours) and on random scalars."""
    import random
    import shutil
    import subprocess

    R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    X = 0xd201000000010000
    X2 = X * X
    rnd = random.Random(77)
    ks = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R - 1) // 2 + 1, (R - 1) // 2 - 1, X2, X2 - 1, X2 + 1, X2 // 2, X2 // 2 + 1,
          X2 // 2 - 1, (1 << 128) - 1, 1 << 128, (1 << 254) + 5]
    for m in (1, 2, 3, 1 << 60, (R // 2) // X2, (R // 2) // X2 - 1):
        for d in (-1, 0, 1):
            ks += [(m * X2 + d) % R, (m * X2 + X2 // 2 + d) % R, (R - m * X2 + d) % R]
    ks += [rnd.randrange(R) for _ in range(20000)]
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "glvcheck.cpp"
    src.write_text(r'''
#include <cstdio>
#include "glv.hip.h"
int main() {
    char line[128];
    while (fgets(line, sizeof line, stdin)) {
        ff::u32 k[8], k1[8], k2[8], n1, n2;
        for (int i = 0; i < 8; ++i) sscanf(line + 8 * (7 - i), "%8x", &k[i]);
        kzgamd::glv_split(k, k1, k2, n1, n2);
        for (int i = 7; i >= 0; --i) printf("%08x", k1[i]);
        printf(" ");
        for (int i = 7; i >= 0; --i) printf("%08x", k2[i]);
        printf(" %u %u\n", n1, n2);
    }
    return 0;
}
''')
    exe = tmp_path / "glvcheck"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], input="".join("%064x\n" % k for k in ks), capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 4 * len(ks)
    bound = int(2 ** 126.5)
    for i, k in enumerate(ks):
        k1, k2, n1, n2 = int(out[4 * i], 16), int(out[4 * i + 1], 16), int(out[4 * i + 2]), int(out[4 * i + 3])
        assert n1 in (0, 1) and n2 in (0, 1)
        assert k1 < bound and k2 < bound, hex(k)
        assert ((-k1 if n1 else k1) + (-k2 if n2 else k2) * X2 - k) % R == 0, hex(k)


@pytest.mark.parametrize("exact", [False, True])
def test_fp28_primitives_at_their_documented_bounds(tmp_path, exact):
    """fp28.hip.h states a contract per primitive (limb and value bounds of the operands, normalisation and value bound
    of the result).  The round-4 g1::dbl bug was a caller outside such a contract; this pins the contracts themselves,
    on the host, at the EDGES of what they allow — values k*p and k*p +- 1, values with an empty top limb, the largest
    value a bound admits, operands with 30-bit limbs — against Python integers: mul / sqr / mul2_inline (Montgomery
    2^392), sub<K> / sub_lazy<K> / neg<K> for every pad (no limb may wrap), is_zero_mod_p with and without its filter
    (-DKZGAMD_FORCE_EXACT_TESTS)."""
    import random
    import shutil
    import subprocess

    P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
    M28 = (1 << 28) - 1
    rnd = random.Random(2828)
    RINV = pow(1 << 392, -1, P)

    def limbs_norm(v):  # normalized representation: limbs 0..12 < 2^28, the rest in the top limb
        assert v < 1 << (364 + 32)
        return [(v >> (28 * i)) & M28 for i in range(13)] + [v >> 364]

    def value(l):
        return sum(x << (28 * i) for i, x in enumerate(l))

    def edge_values(k):  # values in [0, k*p): multiples of p and their neighbours, empty top limb, the maximum, random
        out = [0, 1, k * P - 1, (1 << 364) - 1, 1 << 364, M28]
        for j in range(k):
            out += [j * P, j * P + 1, max(0, j * P - 1)]
        out += [rnd.randrange(k * P) for _ in range(40)] + [rnd.randrange(1 << 364) for _ in range(6)]
        return [v for v in out if v < k * P]

    def lazy(maxlimb_bits):  # a representation with limbs up to maxlimb_bits wide
        return [rnd.randrange(1 << maxlimb_bits) if rnd.random() < 0.8 else (1 << maxlimb_bits) - 1 for _ in range(14)]

    cases = []  # (op, operands as limb lists, checker)

    def fmt(l):
        return " ".join("%x" % x for x in l)

    def check_mont(prod):
        def chk(out):
            assert all(x <= M28 for x in out[:13]), "result not normalized"
            assert value(out) < 2 * P, "result not below 2p"
            assert (value(out) - prod * RINV) % P == 0, "wrong residue"
        return chk

    # ---- mul / sqr / mul2 ----
    for _ in range(300):
        ka, kb = rnd.choice([(2, 2), (10, 6), (16, 4), (32, 2), (64, 1), (8, 8)])
        a, b = rnd.choice(edge_values(ka)), rnd.choice(edge_values(kb))
        cases.append(("mul", [limbs_norm(a), limbs_norm(b)], check_mont(a * b)))
        cases.append(("sqr", [limbs_norm(b)], check_mont(b * b)))
    for _ in range(200):  # operands with 30-bit limbs: value up to ~2^394, the other operand keeps the product below 2^392 p
        a = lazy(30)
        bmax = ((P << 392) // max(value(a), 1)) - 1
        b = rnd.randrange(min(bmax, 2 * P)) if bmax > 0 else 0
        cases.append(("mul", [a, limbs_norm(b)], check_mont(value(a) * b)))
        s = lazy(29)  # sqr of a lazy sum of two normalized values < 2^29 per limb: keep the value product in range
        if value(s) ** 2 < (P << 392):
            cases.append(("sqr", [s], check_mont(value(s) ** 2)))
    for _ in range(100):  # both operands with 30-bit limbs (the value bound leaves room for that in the low half only)
        a, b = lazy(30)[:7] + [0] * 7, lazy(30)[:7] + [0] * 7
        cases.append(("mul", [a, b], check_mont(value(a) * value(b))))
    for _ in range(300):  # mul2: one lazy operand (limbs < 2^28 + 2^29) per product, as its callers pass
        a, c = limbs_norm(rnd.choice(edge_values(2))), limbs_norm(rnd.choice(edge_values(2)))
        b = [rnd.randrange((1 << 28) + (1 << 29)) for _ in range(13)] + [rnd.randrange(0x1a0110 + 0x1a011 * 8)]
        d = [rnd.randrange((1 << 28) + (1 << 29)) for _ in range(13)] + [rnd.randrange(0x1a0110 + 0x1a011 * 8)]
        tot = value(a) * value(b) + value(c) * value(d)
        if tot < (P << 392):
            cases.append(("mul2", [a, b, c, d], check_mont(tot)))
    # ---- sub<K>, sub_lazy<K>, neg<K> ----
    for k in (2, 4, 8, 16, 32):
        for bv in edge_values(k - 1):
            for av in (0, rnd.choice(edge_values(2)), rnd.choice(edge_values(10))):
                want = av + k * P - bv

                def chk_sub(out, want=want):
                    assert all(x <= M28 for x in out[:13]) and value(out) == want

                def chk_lazy(out, want=want):
                    assert all(x < (1 << 28) + (1 << 29) for x in out[:13]) and out[13] < 1 << 31 and value(out) == want

                cases.append(("sub%d" % k, [limbs_norm(av), limbs_norm(bv)], chk_sub))
                cases.append(("subl%d" % k, [limbs_norm(av), limbs_norm(bv)], chk_lazy))
            cases.append(("neg%d" % k, [limbs_norm(bv)], lambda out, w=k * P - bv: (all(x <= M28 for x in out[:13]) and value(out) == w) or (_ for _ in ()).throw(AssertionError("neg"))))
    # ---- is_zero_mod_p: normalized or lazy a with value < 64p ----
    for j in range(64):
        for v, want in ((j * P, 1), (j * P + 1, 0), (j * P + (1 << 364), 0), (j * P + (1 << 200), 0)):
            if j * P <= v < 64 * P and (v != 0 or want):
                cases.append(("iszero", [limbs_norm(v)], lambda out, w=want: out == [w] or (_ for _ in ()).throw(AssertionError("iszero"))))
    for _ in range(200):
        v = rnd.randrange(64 * P)
        cases.append(("iszero", [limbs_norm(v)], lambda out, w=int(v % P == 0): out == [w] or (_ for _ in ()).throw(AssertionError("iszero"))))
    # a lazy (unnormalized) multiple of p: sum of two normalized multiples, limb-wise
    for _ in range(50):
        x, y = limbs_norm(rnd.randrange(30) * P), limbs_norm(rnd.randrange(30) * P)
        cases.append(("iszero", [[p + q for p, q in zip(x, y)]], lambda out: out == [1] or (_ for _ in ()).throw(AssertionError("iszero lazy"))))

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "fp28check.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "fp28.hip.h"
using fp28::Fe;
static Fe rd() { Fe r; for (int i = 0; i < 14; ++i) if (scanf("%x", &r.v[i]) != 1) r.v[i] = 0; return r; }
static void wr(const Fe& a) { for (int i = 0; i < 14; ++i) printf("%x ", a.v[i]); printf("\n"); }
int main() {
    char op[16];
    while (scanf("%15s", op) == 1) {
        if (!strcmp(op, "mul")) { Fe a = rd(), b = rd(); wr(fp28::mul(a, b)); }
        else if (!strcmp(op, "sqr")) { Fe a = rd(); wr(fp28::sqr(a)); }
        else if (!strcmp(op, "mul2")) { Fe a = rd(), b = rd(), c = rd(), d = rd(); wr(fp28::mul2_inline(a, b, c, d)); }
        else if (!strcmp(op, "iszero")) { Fe a = rd(); printf("%d\n", fp28::is_zero_mod_p(a) ? 1 : 0); }
#define SUBS(K) \
        else if (!strcmp(op, "sub" #K)) { Fe a = rd(), b = rd(); wr(fp28::sub<K>(a, b)); } \
        else if (!strcmp(op, "subl" #K)) { Fe a = rd(), b = rd(); wr(fp28::sub_lazy<K>(a, b)); } \
        else if (!strcmp(op, "neg" #K)) { Fe a = rd(); wr(fp28::neg<K>(a)); }
        SUBS(2) SUBS(4) SUBS(8) SUBS(16) SUBS(32)
        else { printf("unknown op %s\n", op); return 1; }
    }
    return 0;
}
''')
    exe = tmp_path / "fp28check"
    subprocess.check_call([cxx, "-O1", "-std=c++17"] + (["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else []) +
                          ["-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    text = "".join(op + " " + " ".join(fmt(l) for l in ops) + "\n" for op, ops, _ in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases) > 3000
    for (op, ops, chk), ln in zip(cases, out):
        got = [int(x, 16) for x in ln.split()]
        try:
            chk(got)
        except AssertionError as e:
            raise AssertionError("%s %s -> %s: %s" % (op, [hex(value(l)) for l in ops], ln, e))


def test_fr29_butterfly_arithmetic_at_its_documented_bounds(tmp_path):
    """fr29.hip.h, the arithmetic of the NTT kernels, on the host against Python integers: mul_signed (result in (-r, r)
    with a signed top limb, for a lazy multiplicand < 64r whose own top limb may be negative), butterfly_signed /
    butterfly_lazy / butterfly_lazy8 (value identities, no limb wraps), one radix-4 round exactly as ntt.hip's ntt_round
    chains them (two butterfly levels, then ONE carry pass: limbs normalised, value grown by < 10r, never negative),
    reduce_lazy on EVERY multiple of r below 64r and its neighbours (its quotient estimate is off by one there or
    nowhere), finish, mul.  The same cases run on the device in tests/test_fr_arith_gpu.py."""
    import shutil
    import subprocess

    import fr29_cases

    cases = fr29_cases.base_cases()  # the construction lives in tests/fr29_cases.py, shared with the device harness
    sval = fr29_cases.sval

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "fr29check.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "fr29.hip.h"
using fr29::Fe;
static Fe rd() { Fe r; for (int i = 0; i < 9; ++i) if (scanf("%x", &r.v[i]) != 1) r.v[i] = 0; return r; }
static void wr(const Fe& a) { for (int i = 0; i < 9; ++i) printf("%x ", a.v[i]); }
static void wr(const ff::Fr& a) { for (int i = 0; i < 8; ++i) printf("%x ", a.v[i]); }
static void bf(Fe& x, Fe& y, const Fe& w) { const Fe t = fr29::mul_signed<true>(y, w); fr29::butterfly_signed(x, y, t); }
int main() {
    char op[16];
    while (scanf("%15s", op) == 1) {
        if (!strcmp(op, "round")) {
            Fe e[4], w[4];
            for (auto& x : e) x = rd();
            for (auto& x : w) x = rd();
            bf(e[0], e[1], w[0]); bf(e[2], e[3], w[1]); bf(e[0], e[2], w[2]); bf(e[1], e[3], w[3]);   // ntt.hip: KZG_BF x 4
            for (auto& x : e) { fr29::norm(x); wr(x); }
        } else if (!strcmp(op, "msig")) { Fe a = rd(), b = rd(); wr(fr29::mul_signed<true>(a, b)); }
        else if (!strcmp(op, "bfs")) { Fe x = rd(), t = rd(), y; fr29::butterfly_signed(x, y, t); wr(x); wr(y); }
        else if (!strcmp(op, "bfl")) { Fe x = rd(), t = rd(), y; fr29::butterfly_lazy(x, y, t); wr(x); wr(y); }
        else if (!strcmp(op, "bfl8")) { Fe x = rd(), t = rd(), y; fr29::butterfly_lazy8(x, y, t); wr(x); wr(y); }
        else if (!strcmp(op, "redl")) { Fe a = rd(); wr(fr29::reduce_lazy(a)); }
        else if (!strcmp(op, "fin")) { Fe a = rd(), m = rd(); wr(fr29::finish(a, m)); }
        else if (!strcmp(op, "mul")) { Fe a = rd(), b = rd(); wr(fr29::mul(a, b)); }
        else { printf("unknown op %s\n", op); return 1; }
        printf("\n");
    }
    return 0;
}
''')
    exe = tmp_path / "fr29check"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    text = "".join(op + " " + " ".join(" ".join("%x" % x for x in l) for l in ops) + "\n" for op, ops, _ in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases) > 5000
    for (op, ops, chk), ln in zip(cases, out):
        got = [int(x, 16) for x in ln.split()]
        try:
            chk(got)
        except AssertionError as e:
            raise AssertionError("%s %s -> %s: %s" % (op, [hex(sval(l)) for l in ops], ln, e))


def test_barrier_audit_on_file_is_the_audit_of_these_sources():
    """DESIGN.md §11 rests on profiles/r06_barrier_audit.txt: every __syncthreads() of the library with the control
    statements around it, each judged workgroup-uniform by hand.  A barrier added, removed, or moved under another
    condition since the audit shows here (line numbers aside), and the conditions the audit accepted are a closed list:
    a new kind of enclosing statement needs a new look, not a regenerated file."""
    import re
    import subprocess

    now = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py")], stderr=subprocess.DEVNULL).decode()
    filed = open(os.path.join(ROOT, "profiles", "r06_barrier_audit.txt")).read()

    def shape(text):
        return [re.sub(r":\d+", "", ln).rstrip() for ln in text.splitlines() if ln.strip()]

    assert shape(now) == shape(filed), "regenerate profiles/r06_barrier_audit.txt (tools/barrier_audit.py) and re-read it"
    assert shape(now)[-1] == "79 barriers"
    assert "79 `__syncthreads()`" in open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    # the enclosing statements the audit found uniform: loops over compile-time or kernel-parameter bounds, conditions
    # on kernel parameters / plan constants / values broadcast through shared memory after a barrier
    inside = sorted({ln.split("inside:", 1)[1].strip() for ln in now.splitlines() if "inside:" in ln})
    for stmt in inside:
        assert not re.search(r"threadIdx|lane|tid\b|__shfl|is_zero|is_inf", stmt), stmt


def test_the_library_reads_four_environment_variables():
    """Configuration is an API (KzgAmdConfig, csrc/config.h), not the process environment: the library sources read the
    four variables DESIGN.md §9 and include/kzg_mi355x.h name, each at one site, and nothing else."""
    import glob

    seen = {}
    for path in glob.glob(os.path.join(ROOT, "rust-kzg_amd", "csrc", "*.h*")):
        for name in re.findall(r'getenv\(\s*"([^"]*)"', open(path).read()):
            seen[name] = seen.get(name, 0) + 1
        assert not re.search(r"getenv\(\s*[^\"\s]", open(path).read()), path  # no computed names
    assert seen == {"KZGAMD_TUNING": 1, "KZGAMD_FBW_MAX_GB": 1, "KZGAMD_VERBOSE": 1, "KZGAMD_DEBUG": 1}
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    for name in seen:
        assert name in design


@pytest.mark.parametrize("exact", [False, True])
def test_g1_point_formulas_against_the_oracle_on_the_host(tmp_path, oracle, exact):
    """g1_28.hip.h (the XYZZ formulas every MSM and G1-transform kernel inlines: madd, dadd, dadd_unequal, dbl, dbl_k,
    mul_small, to_blst_jacobian) compiled for the host and held to the oracle's point arithmetic, with the exceptional
    cases the reference's p1_dadd_affine / p1_dadd handle (kzg/src/msm/pippenger_utils.rs:90-210): the accumulator or the
    addend at infinity, P + P (the doubling branch of an addition), P + (-P); with and without the filter in front of the
    exact zero test (the two builds of the library)."""
    import random
    import shutil
    import subprocess

    import oracle_ffi as O

    L = oracle.lib()
    rnd = random.Random(515)
    g = O.G1()
    L.og1_generator(C.byref(g))

    def comp(p):
        buf = C.create_string_buffer(48)
        L.og1_compress(buf, C.byref(p))
        return buf.raw.hex()

    def mul(p, k):
        r, kf = O.G1(), O.fr_from_int(k % O.R)
        L.og1_mul(C.byref(r), C.byref(p), C.byref(kf))
        return r

    def add(a, b):
        r = O.G1()
        L.og1_add_or_dbl(C.byref(r), C.byref(a), C.byref(b))
        return r

    inf = O.G1()
    cases = []  # (line, expected compressed)
    for it in range(60):
        P = mul(g, rnd.randrange(1, O.R))
        Q = mul(g, rnd.randrange(1, O.R))
        P2, Q2 = mul(P, 2), mul(Q, 2)
        k = rnd.choice([0, 1, 2, 3, 15, 16, 112, 255]) if it % 2 else rnd.randrange(1, 300)
        ks = rnd.choice([0, 1, 2, 3, 5, 64, 0xFFFF, 0x12345])
        rows = [
            ("madd", P, Q, 0, add(P2, Q)), ("madd", P, P2, 0, mul(P, 4)), ("madd", P, mul(P2, O.R - 1), 0, inf),
            ("madd0", P, Q, 0, Q),
            ("dadd", P, Q, 0, add(P2, Q2)), ("dadd", P, P, 0, mul(P, 4)), ("dadd", P, mul(P, O.R - 1), 0, inf),
            ("dadd", inf, Q, 0, Q2), ("dadd", P, inf, 0, P2),
            ("daddu", P, Q, 0, add(P2, Q2)), ("daddu", P, P, 0, mul(P, 4)), ("daddu", P, mul(P, O.R - 1), 0, inf),
            ("dblk", P, inf, k, mul(P, 2 << k)), ("muls", P, inf, ks, mul(P, 2 * ks)),
        ]
        for op, a, b, kk, want in rows:
            cases.append(("%s %s %s %d" % (op, comp(a), comp(b), kk), comp(want)))
    cases.append(("dblk %s %s 7" % (comp(inf), comp(inf)), comp(inf)))
    cases.append(("muls %s %s 9" % (comp(inf), comp(inf)), comp(inf)))

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "g1formulas.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "g1_28.hip.h"
#include "host_g1.h"
using g1::Xyzz;
static bool rd(Xyzz& out) {  // compressed hex -> XYZZ (affine: ZZ = ZZZ = 1), infinity -> all-zero
    char h[128];
    if (scanf("%127s", h) != 1) return false;
    uint8_t in[48];
    for (int i = 0; i < 48; ++i) { unsigned v; sscanf(h + 2 * i, "%2x", &v); in[i] = (uint8_t)v; }
    blst_p1 p;
    if (!kzgamd::host_p1_uncompress(&p, in)) return false;
    const ff::Fp* P = reinterpret_cast<const ff::Fp*>(&p);
    if (P[2].is_zero()) g1::set_inf(out);
    else g1::set_affine(out, fp28::from_blst(P[0]), fp28::from_blst(P[1]));
    return true;
}
static void wr(const Xyzz& a) {
    blst_p1 p;
    g1::to_blst_jacobian(reinterpret_cast<ff::Fp*>(&p), a);
    uint8_t c[48];
    kzgamd::host_p1_compress(c, &p);
    for (int i = 0; i < 48; ++i) printf("%02x", c[i]);
    printf("\n");
}
static void twice(Xyzz& a) { if (!g1::is_inf(a)) g1::dbl(a); }   // a non-trivial ZZ on every operand
int main() {
    char op[16];
    while (scanf("%15s", op) == 1) {
        Xyzz a, b;
        unsigned k;
        if (!rd(a) || !rd(b) || scanf("%u", &k) != 1) { printf("input\n"); return 1; }
        if (!strcmp(op, "madd")) { Xyzz acc = a; twice(acc); g1::madd(acc, b.x, b.y); wr(acc); }
        else if (!strcmp(op, "madd0")) { Xyzz acc; g1::set_inf(acc); g1::madd(acc, b.x, b.y); wr(acc); }
        else if (!strcmp(op, "dadd")) { twice(a); twice(b); g1::dadd(a, b); wr(a); }
        else if (!strcmp(op, "daddu")) { twice(a); twice(b); if (g1::dadd_unequal(a, b)) g1::dbl(a); wr(a); }
        else if (!strcmp(op, "dblk")) { twice(a); g1::dbl_k(a, (int)k); wr(a); }
        else if (!strcmp(op, "muls")) { twice(a); g1::mul_small(a, k); wr(a); }
        else { printf("unknown\n"); return 1; }
    }
    return 0;
}
''')
    exe = tmp_path / "g1formulas"
    subprocess.check_call([cxx, "-O1", "-std=c++17"] + (["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else []) + ["-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], input="\n".join(c[0] for c in cases) + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(cases) > 800
    for (line, want), got in zip(cases, out):
        assert got == want, line.split()[0] + " " + line.split()[-1]


def build_g1io(tmp_path):
    """the stand-alone program over csrc/g1_io.hip.h compiled for the host: per line of compressed hex on stdin `bad` or
    `ok <compressed again> <its double, compressed> <affpt_in_g1>`"""
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "g1io.cpp"
    src.write_text(r'''
#include <cstdio>
#include "g1_28.hip.h"
#include "g1_io.hip.h"
static void hex(const unsigned char* p) { for (int i = 0; i < 48; ++i) printf("%02x", p[i]); }
int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        unsigned char in[48], c[48], c2[48];
        for (int i = 0; i < 48; ++i) { unsigned v; sscanf(line + 2 * i, "%2x", &v); in[i] = (unsigned char)v; }
        g1::AffPt a;
        if (!g1io::uncompress(a, in)) { printf("bad\n"); continue; }
        g1::Xyzz p;
        if (a.flags & 1) g1::set_inf(p);
        else g1::set_affine(p, a.x, a.y);
        g1io::compress(c, p);
        if (!g1::is_inf(p)) g1::dbl(p);
        g1io::compress(c2, p);
        printf("ok ");
        hex(c);
        printf(" ");
        hex(c2);
        printf(" %d\n", g1io::affpt_in_g1(a) ? 1 : 0);
    }
    return 0;
}
''')
    exe = tmp_path / "g1io"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def test_device_g1_serialisation_code_against_the_oracle_on_the_host(tmp_path, oracle):
    """g1_io.hip.h — what k_uncompress / k_decode_check_g1 and the compressed output mode of the MSM's last kernel run per
    point — compiled for the host: the same encodings as the host_g1.h test (valid, outside G1, every invalid class) are
    accepted or refused as the oracle does, accepted ones compress back to themselves, and a point with non-trivial
    ZZ / ZZZ (its double) compresses to the oracle's bytes (the inversion behind it included)."""
    import random
    import shutil
    import subprocess

    import oracle_ffi as O

    L = oracle.lib()
    enc, valid = _g1_encodings(L, O, random.Random(404))
    exe = build_g1io(tmp_path)
    out = subprocess.run([str(exe)], input="\n".join(e.hex() for e in enc) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(enc)
    for i, (e, ln) in enumerate(zip(enc, out)):
        assert (ln != "bad") == (i < valid), (i, e.hex(), ln)
        if ln == "bad":
            continue
        _, again, doubled, in_g1 = ln.split()
        assert again == e.hex(), i
        a, p, d = O.G1Affine(), O.G1(), O.G1()
        assert L.og1_uncompress(C.byref(a), e)
        if not e[0] & 0x40:
            L.og1_from_affine(C.byref(p), C.byref(a))
        L.og1_dbl(C.byref(d), C.byref(p))
        buf = C.create_string_buffer(48)
        L.og1_compress(buf, C.byref(d))
        assert doubled == buf.raw.hex(), i
        assert int(in_g1) == L.og1_in_subgroup(C.byref(p)), (i, e.hex())  # affpt_in_g1, the single-lane membership test
