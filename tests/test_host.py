"""CPU tests: the C-ABI library loads and exports what include/*.h declares; the host parser's
products equal the reference's internals; host-built tables equal the reference's (known answers);
the golden fixtures still decode to the recorded hashes with the reference."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from streams import synth, VARDCT_CASES, ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_library_exports_declared_abi(built):
    import j40_amd
    L = j40_amd.lib()
    declared = set()
    for header, pat in (("include/j40hip.h", r"J40HIP_API[^;]*?\b(j40hip_\w+)\s*\("), ("include/j40.h", r"J40_API[^;]*?\b(j40_\w+)\s*\(")):
        text = open(os.path.join(ROOT, header)).read()
        declared |= set(re.findall(pat, text))
    assert len(declared) >= 35
    for name in sorted(declared):
        assert hasattr(L, name), "libj40hip.so does not export %s" % name


def test_environment_switches_are_the_documented_ones():
    """INTEGRATION.md's "Environment switches" paragraph lists exactly the J40HIP_* variables the library reads, and the tests and
    bench.py set none that it does not read (J40HIP_LIB selects the library itself; J40HIP_API is the headers' export macro)."""
    import glob
    literal = re.compile(r"[\"'](J40HIP_[A-Z0-9_]+)[\"']")
    read = set()
    for pat in ("j40_amd/csrc/*", "j40_amd/csrc/device/*", "j40_amd/*.py"):
        for path in glob.glob(os.path.join(ROOT, pat)):
            if os.path.isfile(path):
                read |= set(literal.findall(open(path, errors="replace").read()))
    read -= {"J40HIP_LIB", "J40HIP_API"}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    para = text[text.index("Environment switches:"):]
    para = para[:para.index("\n\n")]
    documented = set(re.findall(r"J40HIP_[A-Z0-9_]*[A-Z0-9]", para))
    assert len(read) >= 40
    assert read == documented, "read but not documented: %s; documented but not read: %s" % (sorted(read - documented), sorted(documented - read))
    put = set()
    sources = glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "bench.py")]
    for path in sources:
        if os.path.basename(path) != "test_host.py":
            put |= set(literal.findall(open(path).read()))
    put -= {"J40HIP_LIB", "J40HIP_API"}
    assert put and put <= read, "set by tests or bench.py, read by nothing: %s" % sorted(put - read)


def test_public_struct_layout(built):
    import j40_amd
    # j40_image: u32 magic + pointer-sized union; j40_frame: 2 x u32 + pointer; pixels: 3 x i32 + pointer
    assert C.sizeof(j40_amd._Image) == 16 and C.sizeof(j40_amd._FrameHandle) == 16 and C.sizeof(j40_amd._Pixels) == 24


def test_product_fails_loudly_without_gpu(built):
    import j40_amd
    if j40_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    err, rgba = j40_amd.decode(synth("vardct", 264, 200, 11))
    assert err == "!gpu" and rgba is None
    img = j40_amd.from_memory(synth("vardct", 264, 200, 11))
    assert not img.next_frame()
    assert "during j40_next_frame" in img.error_string()
    px, stride, _ = img.frame_pixels_u8x4()
    assert px.shape == (7, 21, 4) and stride == 84  # the reference's "ERR" placeholder (j40.h:8432)
    img.free()
    assert img.error() == "Ufre"   # j40.h:8475-8476: a freed image answers every call with "Ufre"


def test_api_misuse_codes(built):
    import j40_amd
    L = j40_amd.lib()
    img = j40_amd._Image()
    assert j40_amd.err4(L.j40_from_memory(C.byref(img), None, 0, None)) == "Ubf0"
    assert j40_amd.err4(L.j40_error(C.byref(img))) == "Ubf0"
    assert b"`buf` parameter is NULL during j40_from_memory" == L.j40_error_string(C.byref(img))
    L.j40_free(C.byref(img))
    assert j40_amd.err4(L.j40_error(C.byref(img))) == "Ufre"
    assert j40_amd.err4(L.j40_from_file(C.byref(img), b"/nonexistent/file.jxl")) == "open"
    assert L.j40_error_string(C.byref(img)).startswith(b"Failed to open file during j40_from_file: ")
    img2 = j40_amd.from_memory(b"\xff\x0a\x00")
    assert img2.output_format(0x1234, j40_amd.J40_U8X4) == "Uch?"
    img2.free()
    bad = j40_amd.from_memory(b"not a jxl file at all")
    assert not bad.next_frame() and bad.error() == "!jxl"
    assert bad.error_string() == "The JPEG XL signature is not found during j40_next_frame"
    bad.free()


def test_golden_fixtures_pin_the_oracle(ref):
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    assert len(manifest) >= 10
    for name, e in sorted(manifest.items()):
        data = open(os.path.join(GOLDEN, name + ".jxl"), "rb").read()
        assert hashlib.sha256(data).hexdigest() == e["stream_sha256"]
        err, rgba = ref.decode(data)
        if "error" in e:       # a stream the reference refuses: the fixture pins its code
            assert err == e["error"] != "", name
            continue
        if "pinned_by" in e:   # Squeeze: the reference stops with TODO; the fixture holds its decode of the same picture coded without it
            from streams import synth
            assert err == "TODO", name
            err, rgba = ref.decode(synth(e["mode"], e["width"], e["height"], e["seed"], **{k: v for k, v in e["opts"].items() if k != "squeeze"}))
        assert err == "" and sha(rgba) == e["rgba_sha256"], name


def test_generator_is_deterministic(built):
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    for name, e in sorted(manifest.items()):
        data = synth(e["mode"], e["width"], e["height"], e["seed"], **e["opts"])
        assert hashlib.sha256(data).hexdigest() == e["stream_sha256"], name


@pytest.mark.parametrize("name,opts", VARDCT_CASES + [("all_transforms", dict(maxlog=8, bctx=1, presets=2, orders=1))])
def test_host_parse_matches_reference_internals(ref, name, opts):
    import j40_amd
    from refdec import RefStage
    w, h = (776, 520) if name == "all_transforms" else (520, 264)
    data = synth("vardct", w, h, 21, **opts)
    rs = RefStage(ref, data)
    fr = j40_amd.Frame(data, threads=2)
    assert fr.info == rs.info
    for gg in range(rs.info["num_lf_groups"]):
        assert fr.lf_group_info(gg) == rs.lf_group_info(gg)
        for which in range(4):
            assert np.array_equal(fr.plane(gg, which), rs.plane(gg, which)), (gg, which)
        ra, rb = rs.varblocks(gg)
        ma, mb = fr.varblocks(gg)
        assert np.array_equal(ra, ma) and np.array_equal(rb.view(np.uint32), mb.view(np.uint32))
        for c in range(3):
            assert np.array_equal(fr.llf(gg, c).view(np.uint32), rs.llf(gg, c).view(np.uint32)), "LLF coefficients must be bit-identical"
    for idx in range(17):
        assert np.array_equal(fr.dq_matrix(idx).view(np.uint32), rs.dq_matrix(idx).view(np.uint32)), idx
    for p in range(rs.info["num_passes"]):
        for idx in range(13):
            for c in range(3):
                assert np.array_equal(fr.order(p, idx, c), rs.order(p, idx, c))
    assert np.array_equal(fr.block_ctx_map(), rs.block_ctx_map())
    fr.close()
    rs.close()


def test_host_parse_golden_llf(built):
    import j40_amd
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    for name, e in sorted(manifest.items()):
        data = open(os.path.join(GOLDEN, name + ".jxl"), "rb").read()
        if e["mode"] != "vardct":
            continue
        fr = j40_amd.Frame(data)
        ll = [fr.llf(g, c) for g in range(fr.info["num_lf_groups"]) for c in range(3)]
        assert sha(np.concatenate(ll)) == e["llf_sha256"], name
        fr.close()


def test_table_known_answers(ref):
    import j40_amd
    L = j40_amd.lib()
    for i in range(256):
        assert np.float32(L.j40hip_kat_half_secant(i)) == np.float32(ref.lib.ref_kat_half_secant(i))
    for i in range(64):
        assert np.float32(L.j40hip_kat_lf2llf_scale(i)) == np.float32(ref.lib.ref_kat_lf2llf_scale(i))
    for lr, lc in [(3, 3), (4, 4), (5, 5), (3, 4), (3, 5), (4, 5), (6, 6), (5, 6), (7, 7), (6, 7), (8, 8), (7, 8)]:
        a, b = np.zeros(65536, np.int32), np.zeros(65536, np.int32)
        n1 = L.j40hip_kat_natural_order(lr, lc, a.ctypes.data)
        n2 = ref.lib.ref_kat_natural_order(lr, lc, b.ctypes.data)
        assert n1 == n2 == 1 << (lr + lc) and np.array_equal(a[:n1], b[:n2]), (lr, lc)
    for idx in range(17):
        a, b = np.zeros((65536, 3), np.float32), np.zeros((65536, 3), np.float32)
        n1 = L.j40hip_kat_library_dq_matrix(idx, a.ctypes.data)
        n2 = ref.lib.ref_kat_library_dq_matrix(idx, b.ctypes.data)
        assert n1 == n2 > 0 and np.array_equal(a[:n1].view(np.uint32), b[:n2].view(np.uint32)), idx
    rng = np.random.default_rng(5)
    for lr in range(0, 6):
        for lc in range(0, 6):
            if lr == 0 and lc == 0:
                continue
            x = rng.normal(size=(1 << lr) * (1 << lc)).astype(np.float32)
            a, b = x.copy(), x.copy()
            L.j40hip_kat_forward_llf(a.ctypes.data, lr, lc)
            ref.lib.ref_kat_forward_llf(b.ctypes.data, lr, lc)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (lr, lc)


def test_parse_errors_match_reference(ref):
    import j40_amd
    data = bytearray(synth("vardct", 520, 264, 21))
    for cut in (3, 40, 200):
        e1 = ref.decode(bytes(data[:cut]))[0]
        with pytest.raises(j40_amd.J40Error) as ei:
            j40_amd.Frame(bytes(data[:cut]))
        assert ei.value.code == e1 == "shrt"
    assert ref.decode(b"JUNKJUNKJUNK")[0] == "!jxl"
    with pytest.raises(j40_amd.J40Error) as ei:
        j40_amd.Frame(b"JUNKJUNKJUNK")
    assert ei.value.code == "!jxl"


def test_bytes_behind_the_frame_like_the_reference(ref):
    """what follows a frame that decodes cleanly: `excs` for bare codestreams and `shrt` for 1-7 stray bytes behind a container's
    last box -- but only while the reference's 64 KB main buffer still covers the end of the frame (j40__seek_buffer empties it
    otherwise and the final j40__no_more_bytes passes); 8 bytes or more behind a container are taken for a box and skipped"""
    import ctypes as C
    import j40_amd
    L = j40_amd.lib()
    L.j40hip_frame_after_frame_status.restype = C.c_uint32
    L.j40hip_frame_after_frame_status.argtypes = [C.c_void_p]
    cases = [("vardct", 520, 264, dict()), ("vardct", 520, 264, dict(container=1)), ("vardct", 520, 264, dict(container=2)),
             ("modular", 600, 300, dict()), ("modular", 600, 300, dict(container=1)), ("modular", 256, 256, dict()), ("modular", 256, 256, dict(container=1)),
             ("modular", 300, 200, dict(palette=1)), ("modular", 300, 200, dict(container=1, palette=1))]
    for mode, w, h, o in cases:
        data = synth(mode, w, h, 9, **o)
        for n in (0, 1, 3, 7, 8, 12, 40):
            d = data + bytes(range(1, n + 1))
            rerr = ref.decode(d)[0]
            fr = j40_amd.Frame(d)
            code = L.j40hip_frame_after_frame_status(fr.h)
            assert ("" if code == 0 else code.to_bytes(4, "big").decode("latin1")) == rerr, (mode, w, h, o, n, rerr)
            fr.close()


def test_from_file_opens_now_and_reads_at_next_frame_like_the_reference(built, tmp_path):
    """j40_from_file only opens the file (j40.h:8342-8361); the bytes are read by j40_next_frame (j40.h:1241-1256, 1307-1343): a path
    that cannot be opened fails in from_file with `open` and the errno text, a directory opens and then fails to READ (`read`) inside
    j40_next_frame, an empty or truncated file ends in `shrt` there. The reference's own dj40.c, built unchanged against both
    libraries (oracle/Makefile `dropin`), must print the same line and exit the same way -- none of these cases reaches the GPU."""
    import subprocess
    exe_ref, exe_hip = os.path.join(ROOT, "oracle", "_ref", "dj40-ref"), os.path.join(ROOT, "oracle", "_ref", "dj40-hip")
    if not (os.path.exists(exe_ref) and os.path.exists(exe_hip)):
        pytest.skip("oracle/_ref/dj40-* not built (needs the reference sources at build time)")
    from streams import synth
    good = synth("vardct", 520, 264, 300)
    (tmp_path / "empty.jxl").write_bytes(b"")
    (tmp_path / "headers_only.jxl").write_bytes(good[:40])
    (tmp_path / "two_bytes.jxl").write_bytes(good[:2])
    (tmp_path / "not_jxl.jxl").write_bytes(b"GIF89a" + bytes(64))
    (tmp_path / "a_directory").mkdir()
    for name in ("missing.jxl", "a_directory", "empty.jxl", "two_bytes.jxl", "headers_only.jxl", "not_jxl.jxl"):
        runs = [subprocess.run([exe, str(tmp_path / name), str(tmp_path / "out.png")], capture_output=True, text=True, timeout=60) for exe in (exe_ref, exe_hip)]
        assert runs[0].returncode == runs[1].returncode != 0, (name, runs[0].stderr, runs[1].stderr)
        assert runs[0].stderr == runs[1].stderr, (name, runs[0].stderr, runs[1].stderr)
    msg = subprocess.run([exe_hip, str(tmp_path / "a_directory"), str(tmp_path / "out.png")], capture_output=True, text=True).stderr
    assert "(read)" in msg and "j40_next_frame" in msg, msg


def test_streamed_parse_reads_only_what_it_asked_for_and_gives_the_same_frame(built):
    """SURVEY.md 8f-3 (the reference's refillable source, j40.h:1220-1386, 1676-1812): j40hip_frame_parse_streamed parses while the
    bytes arrive. The buffer here starts as rubbish and fills only as far as the parser's need(n) calls say (rounded up to 64 bytes or
    4 KB): the parsed frame -- headers, TOC, LfGlobal, HfGlobal, every LfGroup's planes and varblocks, serialised by lf_bundle -- must
    be the one the whole buffer gives; when the host's parse returns, the pass-group sections (most of the file) have not been asked
    for; truncated and damaged streams fail with the whole-buffer parse's code; containers are parsed once complete"""
    import j40_amd
    from streams import synth
    cases = [("vardct", 2600, 2100, 41, dict()), ("vardct", 1920, 1080, 34, dict(forward=1)), ("vardct", 520, 264, 7, dict(icc=700)), ("vardct", 264, 200, 11, dict()),
             ("vardct", 776, 520, 31, dict(passes=2, permute=1)), ("vardct", 520, 264, 8, dict(container=2))]
    for mode, w, h, seed, opts in cases:
        data = synth(mode, w, h, seed, **opts)
        whole = j40_amd.Frame(data, threads=3)
        want = whole.lf_bundle()
        whole.close()
        for step in (64, 4096):
            log = []
            fr = j40_amd.Frame.parse_streamed(data, step=step, threads=3, log=log)
            assert fr.lf_bundle() == want, (w, h, opts, step)
            if not opts.get("container") and w >= 1900 and not opts.get("permute"):
                assert fr.revealed < len(data) // 2, (fr.revealed, len(data))   # the coefficient sections were never asked for
                assert log[0] == 2 and len(log) >= 4   # the signature, the headers' prefix, the global sections, the LfGroup sections
            fr.close()
    data = synth("vardct", 2600, 2100, 41)
    rng = np.random.default_rng(5)
    for trial in range(24):
        bad = bytearray(data)
        if trial % 3 == 0:
            bad = bad[: int(rng.integers(2, len(data) // 8))]
        else:
            bad[int(rng.integers(2, len(data) // 8))] ^= 1 << int(rng.integers(0, 8))
        codes = []
        for parse in (lambda b: j40_amd.Frame(b, threads=2), lambda b: j40_amd.Frame.parse_streamed(b, step=64, threads=2)):
            try:
                f = parse(bytes(bad)); f.close(); codes.append("")
            except j40_amd.J40Error as e:
                codes.append(e.code)
        assert codes[0] == codes[1], (trial, codes)

