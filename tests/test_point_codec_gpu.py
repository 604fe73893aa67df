"""The batched codec calls (codec.hip) through the C ABI, on both library flavours: kzgamd_g1_uncompress_batch,
kzgamd_g1_compress_batch, kzgamd_g1_to_affine_batch, kzgamd_g2_uncompress_batch, kzgamd_g2_compress_batch, and the
host's kzgamd_p2_in_g2.

Anchors, none of them the code under test: the CPU oracle (og1_uncompress / og1_compress / og1_to_affine) for G1, the
host's kzgamd_p2_uncompress / kzgamd_p2_compress and tests/codec_model.py for G2, and the classes of the two catalogues
(tests/g1_encodings.py, tests/g2_encodings.py: Python integers) for every status.

Counts: 1, 3, 4, 5, 63, 64, 65, 257 are the row, wave and block edges of the two G1 decode forms (four points per wave;
64 lanes per block), 4099 is just above the count where the decode changes from the wide form to a lane per point;
1, 63, 64, 65, 1025 the wave and block edges of the G1 output kernel, which takes one point per lane up to 2^16 points of a
launch, four up to 2^18 and eight above: 2^16 + 1 points, and 2^18 + 1 under codec_slice=2^19, run the two chunked forms
against the oracle's answers for a 41-point pattern (41 is odd, so every chunk of 4 or 8 holds another mix: identities
only, one identity, none).  1, 63, 64, 65, 130 are the edges of the G2 kernels (a lane per point, 64 per block).

Files: kzgamd_read_trusted_setup_file / kzgamd_write_trusted_setup_file on the golden setup (read == the oracle's decode,
written again == the golden text), on generated setups of 8 + 3 and of 4096 + 65 points (the latter loaded through the
c-kzg surface and held to the oracle's commitment under the same text), and the three refusals (codes 1, 2, 3)."""
import ctypes as C
import os
import random

import pytest

import codec_model as M
import g1_encodings as E
import g2_encodings as E2
import oracle_ffi as O
import setup_model as S

pytestmark = pytest.mark.gpu
P = M.P
ONE_MONT = ((1 << 384) % P).to_bytes(48, "little")
INF1 = b"\xc0" + bytes(47)
INF2 = b"\xc0" + bytes(95)
_ref = {}


def fr_bulk(kzg, vals):
    raw = b"".join(((v << 256) % M.R).to_bytes(32, "little") for v in vals)
    arr = (kzg.BlstFr * max(len(vals), 1))()
    C.memmove(arr, raw, len(raw))
    return arr


def cycle(entries, n, start=0):
    return [entries[(start + i) % len(entries)] for i in range(n)]


# ---------------------------------------------------------------- G1 references (the oracle)
def oracle_g1(b):
    """the 144 bytes of the oracle's decode of a valid encoding (Z = one; the identity all-zero)"""
    if b not in _ref:
        L = O.lib()
        a, g = O.G1Affine(), O.G1()
        assert L.og1_uncompress(C.byref(a), b) == 1, b.hex()
        if b == INF1:
            _ref[b] = bytes(144)
        else:
            L.og1_from_affine(C.byref(g), C.byref(a))
            _ref[b] = bytes(g)
            assert _ref[b][96:] == ONE_MONT
    return _ref[b]


def oracle_compress(p144):
    L = O.lib()
    g = O.G1()
    C.memmove(C.byref(g), p144, 144)
    if L.og1_is_inf(C.byref(g)):
        return INF1, bytes(96)
    out = C.create_string_buffer(48)
    L.og1_compress(out, C.byref(g))
    a = O.G1Affine()
    L.og1_to_affine(C.byref(a), C.byref(g))
    return out.raw, bytes(a)


def check_g1_parse(kzg, entries, check, config=None):
    data = b"".join(b for _, b, _ in entries)
    pts, status, rc = kzg.g1_uncompress_batch(data, check_subgroup=check, config=config)
    want = [cls if check or cls != 2 else 0 for _, _, cls in entries]
    assert list(status) == want, [(n, s, w) for (n, _, _), s, w in zip(entries, status, want) if s != w][:5]
    assert rc == (1 if any(want) else 0)
    for i, ((name, b, cls), w) in enumerate(zip(entries, want)):
        got = bytes(pts[i])
        if w != 0:
            assert got == bytes(144), (name, "a refused entry is all-zero")
        else:
            assert got == oracle_g1(b), (name, i)
    return pts, status, rc


@pytest.mark.parametrize("check", [0, 1])
def test_g1_parse_the_catalogue_at_every_edge_of_the_two_decode_forms(kzg, check):
    cat = list(E.catalogue())
    check_g1_parse(kzg, cat, check)
    for n in (1, 3, 4, 5, 63, 64, 65, 257):
        for start in ((0, 29, 40) if n < 6 else (n % 7,)):  # a valid, an outside and a malformed entry first
            check_g1_parse(kzg, cycle(cat, n, start), check)
    accepted = cycle(E.by_class(0), 5)
    pts, status, rc = kzg.g1_uncompress_batch(b"".join(b for _, b in accepted), check_subgroup=check)
    assert rc == 0 and list(status) == [0] * 5


@pytest.mark.parametrize("check", [0, 1])
def test_g1_parse_just_above_the_wide_decode_limit(kzg, check):
    check_g1_parse(kzg, cycle(list(E.catalogue()), 4096 + 3, 11), check)


# ---------------------------------------------------------------- G1 out
def g1_inputs(kzg, n, rnd):
    """n blst_p1: Z = 1 (the oracle's decode), arbitrary Z (kzgamd_g1_mul_batch), identities with junk in X and Y; by
    chunks of 8: identities only, one identity, none, one point among identities, then mixed"""
    valid = [b for _, b in E.by_class(0) if b != INF1]
    scalars = [rnd.randrange(1, M.R) for _ in range(32)]
    if "mul" not in _ref:
        _ref["mul"] = [bytes(p) for p in kzg.g1_mul_batch(fr_bulk(kzg, scalars), len(scalars))]
        assert any(p[96:] != ONE_MONT for p in _ref["mul"])
    out = []
    for i in range(n):
        chunk, j = (i // 8) % 5, i % 8
        ident = chunk == 0 or (chunk == 1 and j == 3) or (chunk == 3 and j != 5) or (chunk == 4 and rnd.random() < 0.3)
        if ident:
            out.append(rnd.randbytes(96) + bytes(48))
        elif i % 3 == 0:
            out.append(oracle_g1(valid[i % len(valid)]))
        else:
            out.append(_ref["mul"][i % len(scalars)])
    if n == 1:
        out = [_ref["mul"][0]]
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_g1_compress_and_to_affine_of_jacobian_points(kzg, n):
    rnd = random.Random(n)
    pts = g1_inputs(kzg, n, rnd)
    buf = (kzg.BlstP1 * n)()
    C.memmove(buf, b"".join(pts), 144 * n)
    want = [oracle_compress(p) for p in pts]
    got = kzg.g1_compress_batch(buf, n)
    aff = bytes(kzg.g1_to_affine_batch(buf, n))
    for i in range(n):
        assert got[48 * i:48 * i + 48] == want[i][0], ("compress", i)
        assert aff[96 * i:96 * i + 96] == want[i][1], ("to_affine", i)
    if n > 8:
        assert got[:48 * 8] == INF1 * 8 and aff[:96 * 8] == bytes(96 * 8)  # a chunk of identities only


@pytest.mark.parametrize("n,slice_points", [(1 << 16, None), ((1 << 16) + 1, None), (1 << 18, None), ((1 << 18) + 1, 1 << 19)])
def test_g1_output_on_either_side_of_the_counts_where_the_chunk_length_changes(kzg, n, slice_points):
    rnd = random.Random(41)
    pattern = g1_inputs(kzg, 41, rnd)
    assert sum(1 for p in pattern[:8] if p[96:] == bytes(48)) == 8 and sum(1 for p in pattern[8:16] if p[96:] == bytes(48)) == 1
    want = [oracle_compress(p) for p in pattern]
    reps = n // 41 + 1
    buf = (kzg.BlstP1 * n)()
    C.memmove(buf, (b"".join(pattern) * reps)[:144 * n], 144 * n)
    cfg = kzg.make_config(tuning="codec_slice=%d" % slice_points) if slice_points else None
    assert kzg.codec_info() == 1 << 18  # the default slice: a launch above it needs the key
    assert kzg.g1_compress_batch(buf, n, config=cfg) == (b"".join(w[0] for w in want) * reps)[:48 * n]
    assert bytes(kzg.g1_to_affine_batch(buf, n, config=cfg)) == (b"".join(w[1] for w in want) * reps)[:96 * n]


def golden_tokens(trusted_setup_text):
    tok = trusted_setup_text.split()
    n1, n2 = int(tok[0]), int(tok[1])
    assert (n1, n2) == (4096, 65)
    return tok[2:2 + n1], tok[2 + n1:2 + n1 + n2], tok[2 + n1 + n2:2 + 2 * n1 + n2]


def test_golden_setup_g1_points_round_trip(kzg, trusted_setup_text):
    lag, _, mono = golden_tokens(trusted_setup_text)
    data = bytes.fromhex((b"".join(lag) + b"".join(mono)).decode())
    assert len(data) == 8192 * 48
    pts, status, rc = kzg.g1_uncompress_batch(data, check_subgroup=True)
    assert rc == 0 and status == bytes(8192)
    assert bytes(pts[5]) == oracle_g1(data[5 * 48:6 * 48]) and bytes(pts[8191]) == oracle_g1(data[8191 * 48:])
    assert kzg.g1_compress_batch(pts, 8192) == data


# ---------------------------------------------------------------- G2
def host_g2(kzg, b):
    """the host's decode of a valid encoding, compressed again by the host"""
    if ("g2", b) not in _ref:
        _ref[("g2", b)] = kzg.p2_compress(kzg.p2_uncompress(b))
        assert _ref[("g2", b)] == b == M.compress(M.decode(b))
    return _ref[("g2", b)]


def check_g2_parse(kzg, entries, check, config=None):
    data = b"".join(b for _, b, _ in entries)
    pts, status, rc = kzg.g2_uncompress_batch(data, check_subgroup=check, config=config)
    want = [cls if check or cls != 2 else 0 for _, _, cls in entries]
    assert list(status) == want, [(n, s, w) for (n, _, _), s, w in zip(entries, status, want) if s != w][:5]
    assert rc == (1 if any(want) else 0)
    for i, ((name, b, cls), w) in enumerate(zip(entries, want)):
        got = bytes(pts[i])
        if w != 0 or b == INF2:
            assert got == bytes(288), (name, "a refused entry and the identity are all-zero")
        else:
            assert got[192:] == ONE_MONT + bytes(48), (name, "Z = 1")
            assert kzg.p2_compress(pts[i]) == host_g2(kzg, b), (name, i)
            x, y = M.decode(b)
            mont = lambda v: (v * (1 << 384) % P).to_bytes(48, "little")
            assert got[:192] == mont(x[0]) + mont(x[1]) + mont(y[0]) + mont(y[1]), (name, "canonical coordinates")
    return pts, status, rc


@pytest.mark.parametrize("check", [0, 1])
def test_g2_parse_the_catalogue(kzg, check):
    cat = list(E2.catalogue())
    check_g2_parse(kzg, cat, check)
    for n in (1, 63, 64, 65, 130):
        for start in ((0, 40, 60) if n == 1 else (n % 5,)):
            check_g2_parse(kzg, cycle(cat, n, start), check)


def test_host_p2_in_g2_on_the_catalogue(kzg):
    seen = set()
    for name, b, cls in E2.catalogue():
        if cls != 1:
            assert kzg.p2_in_g2(kzg.p2_uncompress(b)) == (cls == 0), name
            seen.add(cls)
    assert seen == {0, 2}
    assert kzg.lib().kzgamd_p2_in_g2(None) == -1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_g2_compress_of_jacobian_points(kzg, n):
    rnd = random.Random(n)
    if "mul2" not in _ref:
        scalars = [rnd.randrange(1, M.R) for _ in range(24)]
        _ref["mul2"] = [bytes(p) for p in kzg.g2_mul_batch(fr_bulk(kzg, scalars), len(scalars))]
        assert any(p[192:] != ONE_MONT + bytes(48) for p in _ref["mul2"])
    outside = [bytes(kzg.p2_uncompress(b)) for _, b in E2.by_class(2)[:6]]
    pts = []
    for i in range(n):
        if n > 1 and i % 5 == 1:
            pts.append(rnd.randbytes(192) + bytes(96))  # the identity with junk in X and Y
        elif i % 7 == 3:
            pts.append(outside[i % len(outside)])
        else:
            pts.append(_ref["mul2"][i % len(_ref["mul2"])])
    buf = (kzg.BlstP2 * n)()
    C.memmove(buf, b"".join(pts), 288 * n)
    got = kzg.g2_compress_batch(buf, n)
    for i in range(n):
        want = INF2 if pts[i][192:] == bytes(96) else kzg.p2_compress(buf[i])
        assert got[96 * i:96 * i + 96] == want, i


def test_golden_setup_g2_points_round_trip(kzg, trusted_setup_text):
    _, g2, _ = golden_tokens(trusted_setup_text)
    data = bytes.fromhex(b"".join(g2).decode())
    pts, status, rc = kzg.g2_uncompress_batch(data, check_subgroup=True)
    assert rc == 0 and status == bytes(65)
    assert kzg.g2_compress_batch(pts, 65) == data
    assert bytes(pts[0]) == bytes(kzg.p2_generator())


# ---------------------------------------------------------------- slices, arguments
def test_slices_give_the_results_of_the_default_slice_and_an_unknown_key_fails(kzg):
    assert kzg.codec_info() >= 4096 and kzg.codec_info() & (kzg.codec_info() - 1) == 0
    cfg = kzg.make_config(tuning="codec_slice=64")
    n = 129
    c1, c2 = cycle(list(E.catalogue()), n, 5), cycle(list(E2.catalogue()), n, 5)
    p1, s1, r1 = check_g1_parse(kzg, c1, 1)
    q1, t1, u1 = check_g1_parse(kzg, c1, 1, config=cfg)
    assert (bytes(p1), s1, r1) == (bytes(q1), t1, u1)
    p2, s2, r2 = check_g2_parse(kzg, c2, 1)
    q2, t2, u2 = check_g2_parse(kzg, c2, 1, config=cfg)
    assert (bytes(p2), s2, r2) == (bytes(q2), t2, u2)
    assert kzg.g1_compress_batch(p1, n) == kzg.g1_compress_batch(p1, n, config=cfg)
    assert bytes(kzg.g1_to_affine_batch(p1, n)) == bytes(kzg.g1_to_affine_batch(p1, n, config=cfg))
    assert kzg.g2_compress_batch(p2, n) == kzg.g2_compress_batch(p2, n, config=cfg)
    L = kzg.lib()
    out1, out2, by = (kzg.BlstP1 * n)(), (kzg.BlstP2 * n)(), C.create_string_buffer(96 * n)
    for tuning in ("mul_slice=64", "codec_slice=63", "codec_slice=32", "codec_slice=64;wide_check=1"):
        bad = kzg._cfgp(kzg.make_config(tuning=tuning))
        assert L.kzgamd_g1_uncompress_batch(out1, None, by, n, 1, bad) == -2, tuning
        assert L.kzgamd_g2_uncompress_batch(out2, None, by, 1, 1, bad) == -2, tuning
        assert L.kzgamd_g1_compress_batch(by, p1, n, bad) == -2, tuning
        assert L.kzgamd_g1_to_affine_batch(by, p1, 1, bad) == -2, tuning
        assert L.kzgamd_g2_compress_batch(by, p2, 1, bad) == -2, tuning


def test_null_arguments_an_empty_call_and_a_null_status(kzg):
    L = kzg.lib()
    p1, p2 = (kzg.BlstP1 * 2)(), (kzg.BlstP2 * 2)()
    by = C.create_string_buffer(b"\xa5" * 192, 192)
    st = C.create_string_buffer(b"\xa5" * 2, 2)
    C.memset(p1, 0xa5, C.sizeof(p1))
    C.memset(p2, 0xa5, C.sizeof(p2))
    poisoned = (bytes(p1), bytes(p2), by.raw, st.raw)
    assert L.kzgamd_g1_compress_batch(None, p1, 1, None) == -1 and L.kzgamd_g1_compress_batch(by, None, 1, None) == -1
    assert L.kzgamd_g1_to_affine_batch(None, p1, 1, None) == -1 and L.kzgamd_g1_to_affine_batch(by, None, 1, None) == -1
    assert L.kzgamd_g2_compress_batch(None, p2, 1, None) == -1 and L.kzgamd_g2_compress_batch(by, None, 1, None) == -1
    assert L.kzgamd_g1_uncompress_batch(None, st, by, 1, 1, None) == -1 and L.kzgamd_g1_uncompress_batch(p1, st, None, 1, 1, None) == -1
    assert L.kzgamd_g2_uncompress_batch(None, st, by, 1, 1, None) == -1 and L.kzgamd_g2_uncompress_batch(p2, st, None, 1, 1, None) == -1
    # n == 0: nothing is written and the pointers are not looked at
    assert L.kzgamd_g1_compress_batch(by, p1, 0, None) == 0 and L.kzgamd_g1_compress_batch(None, None, 0, None) == 0
    assert L.kzgamd_g1_to_affine_batch(by, p1, 0, None) == 0 and L.kzgamd_g2_compress_batch(by, p2, 0, None) == 0
    assert L.kzgamd_g1_uncompress_batch(p1, st, by, 0, 1, None) == 0 and L.kzgamd_g2_uncompress_batch(p2, st, by, 0, 1, None) == 0
    assert L.kzgamd_g2_uncompress_batch(None, None, None, 0, 0, None) == 0
    assert (bytes(p1), bytes(p2), by.raw, st.raw) == poisoned
    # a NULL status
    g1 = b"".join(b for _, b in E.by_class(0)[:2])
    assert L.kzgamd_g1_uncompress_batch(p1, None, g1, 2, 1, None) == 0 and bytes(p1[1]) == oracle_g1(g1[48:])
    assert L.kzgamd_g1_uncompress_batch(p1, None, g1[:48] + bytes(48), 2, 1, None) == 1 and bytes(p1[1]) == bytes(144)
    g2 = b"".join(b for _, b in E2.by_class(0)[1:3])
    assert L.kzgamd_g2_uncompress_batch(p2, None, g2, 2, 1, None) == 0 and kzg.p2_compress(p2[1]) == g2[96:]
    assert L.kzgamd_g2_uncompress_batch(p2, None, g2[:96] + bytes(96), 2, 0, None) == 1 and bytes(p2[1]) == bytes(288)


# ---------------------------------------------------------------- setup files
def test_golden_setup_file_reads_as_the_oracle_decodes_it_and_writes_back_to_the_same_text(kzg, trusted_setup_text, tmp_path):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trusted_setup.txt")
    mono, lag, g2, n1, n2, rc = kzg.read_trusted_setup_file(golden)
    assert (n1, n2, rc) == (4096, 65, 0)
    lag_t, g2_t, mono_t = golden_tokens(trusted_setup_text)
    for i in list(range(0, 4096, 97)) + [4095]:
        assert bytes(lag[i]) == oracle_g1(bytes.fromhex(lag_t[i].decode())), ("lagrange", i)
        assert bytes(mono[i]) == oracle_g1(bytes.fromhex(mono_t[i].decode())), ("monomial", i)
    assert kzg.g1_compress_batch(lag, 4096) == bytes.fromhex(b"".join(lag_t).decode())
    assert kzg.g1_compress_batch(mono, 4096) == bytes.fromhex(b"".join(mono_t).decode())
    for i in range(65):
        assert kzg.p2_compress(g2[i]) == bytes.fromhex(g2_t[i].decode()) and bytes(g2[i])[192:] == ONE_MONT + bytes(48), i
    out = tmp_path / "again.txt"
    kzg.write_trusted_setup_file(str(out), mono, lag, g2, 4096, 65)
    assert out.read_bytes() == trusted_setup_text


def test_generated_small_setup_round_trips_through_a_file(kzg, tmp_path):
    fs = kzg.FFTSettings(3)
    try:
        mono, lag, g2 = kzg.generate_trusted_setup(8, S.SECRETS["fk20"], num_g2=3, fft_settings=fs)
    finally:
        fs.close()
    path = tmp_path / "small.txt"
    kzg.write_trusted_setup_file(str(path), mono, lag, g2, 8, 3)
    lines = path.read_bytes().split(b"\n")
    assert lines[:2] == [b"8", b"3"] and [len(x) for x in lines[2:]] == [96] * 8 + [192] * 3 + [96] * 8
    assert path.read_bytes() == path.read_bytes().lower() and not path.read_bytes().endswith(b"\n")
    m2, l2, q2, n1, n2, rc = kzg.read_trusted_setup_file(str(path), config=kzg.make_config(tuning="codec_slice=64"))
    assert (n1, n2, rc) == (8, 3, 0)
    for i in range(8):  # the same points, normalised
        assert oracle_compress(bytes(m2[i])) == oracle_compress(bytes(mono[i])) and bytes(m2[i])[96:] == ONE_MONT
        assert oracle_compress(bytes(l2[i])) == oracle_compress(bytes(lag[i]))
    for i in range(3):
        assert kzg.p2_compress(q2[i]) == kzg.p2_compress(g2[i])
    # other whitespace, as the loader takes it; and sections that are not wanted
    spaced = tmp_path / "spaced.txt"
    spaced.write_bytes(b"  8\t3\r\n" + b" \n\n".join(lines[2:]) + b"\n\n")
    m3, l3, q3, n1, n2, rc = kzg.read_trusted_setup_file(str(spaced))
    assert (n1, n2, rc) == (8, 3, 0) and (bytes(m3), bytes(l3), bytes(q3)) == (bytes(m2), bytes(l2), bytes(q2))
    L = kzg.lib()
    c1, c2, only = C.c_size_t(0), C.c_size_t(3), (kzg.BlstP2 * 3)()
    f = kzg._fopen(str(path))
    try:
        assert L.kzgamd_read_trusted_setup_file(f, None, None, only, C.byref(c1), C.byref(c2), None) == 0
    finally:
        kzg._libc.fclose(f)
    assert (c1.value, c2.value) == (8, 3) and bytes(only) == bytes(q2)
    assert L.kzgamd_read_trusted_setup_file(None, None, None, None, C.byref(c1), C.byref(c2), None) == -1
    assert L.kzgamd_write_trusted_setup_file(None, mono, lag, g2, 8, 3, None) == -1


def test_generated_4844_setup_written_to_a_file_loads_and_commits_as_the_oracle_does(kzg, tmp_path):
    fs = kzg.FFTSettings(12)
    try:
        mono, lag, g2 = kzg.generate_trusted_setup(4096, S.SECRETS["fk20"], num_g2=65, fft_settings=fs)
    finally:
        fs.close()
    path = tmp_path / "generated.txt"
    kzg.write_trusted_setup_file(str(path), mono, lag, g2, 4096, 65)
    text = path.read_bytes()
    settings = kzg.KZGSettings.from_file(str(path), config=kzg.make_config(no_tables=True))
    rc, osettings = O.load_settings(text)
    assert rc == 0
    rnd = random.Random(4844)
    blob = b"".join(rnd.randrange(M.R).to_bytes(32, "big") for _ in range(4096))
    want = C.create_string_buffer(48)
    assert O.lib().oblob_to_kzg_commitment(want, blob, C.byref(osettings)) == 0
    assert kzg.blob_to_kzg_commitment(blob, settings) == want.raw
    O.lib().ofree_trusted_setup(C.byref(osettings))


def test_setup_file_refusals(kzg, trusted_setup_text, tmp_path):
    lag_t, g2_t, mono_t = golden_tokens(trusted_setup_text)
    outside1 = E.by_class(2)[0][1].hex().encode()
    outside2 = E2.by_class(2)[0][1].hex().encode()

    def file_of(n1, n2, lag, g2, mono, name):
        p = tmp_path / name
        p.write_bytes(b"\n".join([str(n1).encode(), str(n2).encode()] + lag + g2 + mono))
        return str(p)

    ok = file_of(4, 2, lag_t[:4], g2_t[:2], mono_t[:4], "ok.txt")
    assert kzg.read_trusted_setup_file(ok)[3:] == (4, 2, 0)
    # 3: a point outside the subgroup in either group, a malformed point; the others are written, it is all-zero
    for name, lag, g2, mono in (("g1", lag_t[:3] + [outside1], g2_t[:2], mono_t[:4]), ("g2", lag_t[:4], [g2_t[0], outside2], mono_t[:4]),
                                ("mono", lag_t[:4], g2_t[:2], [b"00" * 48] + mono_t[1:4])):
        m, l, q, n1, n2, rc = kzg.read_trusted_setup_file(file_of(4, 2, lag, g2, mono, name + ".txt"))
        assert (n1, n2, rc) == (4, 2, 3), name
        assert bytes(l[0]) == oracle_g1(bytes.fromhex(lag_t[0].decode())) and bytes(m[1]) == oracle_g1(bytes.fromhex(mono_t[1].decode()))
        assert (bytes(l[3]) == bytes(144)) == (name == "g1") and (bytes(q[1]) == bytes(288)) == (name == "g2")
        assert (bytes(m[0]) == bytes(144)) == (name == "mono")
    # 2: a capacity too small; the counts are still written
    for cap in ((3, 2), (4, 1), (0, 0)):
        m, l, q, n1, n2, rc = kzg.read_trusted_setup_file(ok, capacity=cap)
        assert (n1, n2, rc) == (4, 2, 2), cap
        assert bytes(m) == bytes(144 * max(cap[0], 1)) and bytes(q) == bytes(288 * max(cap[1], 1))
    # 1: malformed text
    bad = {"no counts": b"", "one count": b"4\n", "a count that is no number": b"four\n2\n" + b"\n".join(lag_t[:4]),
           "a point short": b"\n".join([b"4", b"2"] + lag_t[:4] + g2_t[:2] + mono_t[:3]),
           "a letter that is no hex digit": b"\n".join([b"4", b"2"] + lag_t[:3] + [b"zz" + lag_t[3][2:]] + g2_t[:2] + mono_t[:4]),
           "counts the text cannot hold": b"\n".join([b"400000000000", b"2"] + lag_t[:4] + g2_t[:2] + mono_t[:4])}
    for name, text in bad.items():
        p = tmp_path / "bad.txt"
        p.write_bytes(text)
        assert kzg.read_trusted_setup_file(str(p))[5] == 1, name
        assert kzg.read_trusted_setup_file(str(p), capacity=(4, 2))[5] == 1, name
