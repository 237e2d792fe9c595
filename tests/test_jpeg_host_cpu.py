"""The JPEG host stage (pg_jpeg_probe / pg_jpeg_plan / pg_jpeg_entropy_decode, pigeon_amd/csrc/jpeg_entropy.h) through ctypes, no GPU:
coefficients, tables and descriptors against the numpy restatement as integers, the plan against pg_prep_ragged_plan, refusals by
reason, damaged files, and the same damaged files through a stand-alone program built with the host compiler's sanitizers."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jpegref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(hip_lib, golden_dir):
    from pigeon_amd import _lib, hip_ops
    z = np.load(os.path.join(golden_dir, "jpeg_fixtures.npz"))
    off, shapes = z["file_off"], z["shapes"]
    files = [z["files"][off[i]:off[i + 1]].tobytes() for i in range(len(shapes))]
    names, refused = [str(n) for n in z["names"]], [str(r) for r in z["refused"]]
    return dict(ops=hip_ops, lib=_lib, names=names, files=files, refused=refused, shapes=[(int(h), int(w)) for h, w in shapes],
                ok=[i for i, r in enumerate(refused) if not r])


def _plan(fx, files):
    ops = fx["ops"]
    return ops.jpeg_plan([ops.jpeg_probe(f) for f in files])


@pytest.fixture(scope="module")
def reference(fx):
    """The restatement's header and coefficients of every supported fixture, computed once."""
    out = {}
    for i in fx["ok"]:
        h = R.parse(fx["files"][i])
        out[i] = (h, R.entropy_decode(fx["files"][i], h))
    return out


@pytest.mark.parametrize("threads", [1, 16])
def test_coefficients_tables_and_descriptors_equal_the_restatement(fx, reference, threads):
    ops = fx["ops"]
    files = [fx["files"][i] for i in fx["ok"]]
    plan = _plan(fx, files)
    coef = torch.full((plan.coef_bytes,), 0x5A, dtype=torch.uint8)         # (the decoder zeroes its regions itself)
    ops.jpeg_entropy_decode(files, plan, coef, threads=threads)
    c = coef.numpy()
    shapes = [(h["height"], h["width"], h["ncomp"], h["hs"], h["vs"]) for h, _ in (reference[i] for i in fx["ok"])]
    lay, (coef_bytes, ws_bytes) = R.layout(shapes)
    assert (plan.coef_bytes, plan.workspace_bytes) == (coef_bytes, ws_bytes)
    for k, i in enumerate(fx["ok"]):
        h, want = reference[i]
        it, name = plan.items[k], fx["names"][i]
        assert (it.height, it.width, it.ncomp, it.hs, it.vs) == shapes[k], name
        co, po, grid = lay[k]
        assert list(it.coef_off)[:it.ncomp] == co[:it.ncomp] and list(it.plane_off)[:it.ncomp] == po[:it.ncomp], name
        assert [(it.bw[j], it.bh[j]) for j in range(it.ncomp)] == grid, name
        assert list(it.qsel)[:it.ncomp] == [cc[3] for cc in h["comps"]], name
        assert np.array_equal(np.ctypeslib.as_array(it.qt).reshape(4, 64), R.quant_natural(h)), name
        for j in range(it.ncomp):
            nb = it.bw[j] * it.bh[j]
            got = c[it.coef_off[j]:it.coef_off[j] + nb * 128].view(np.int16).reshape(nb, 64)
            assert np.array_equal(got, want[j]), f"{name}: component {j}, first differing block {np.argwhere((got != want[j]).any(1))[:1]}"
    # the descriptors travel in the buffer's head
    assert bytes(c[:plan.header_bytes]) == bytes(plan.header())


def test_plan_offsets_equal_the_ragged_resize_plan(fx):
    ops = fx["ops"]
    plan = _plan(fx, [fx["files"][i] for i in fx["ok"]])
    sizes = [fx["shapes"][i] for i in fx["ok"]]
    want = ops.ragged_plan(sizes)
    assert plan.prep.packed_bytes == want.packed_bytes and plan.prep.workspace_bytes == want.workspace_bytes
    assert bytes(plan.prep.header()) == bytes(want.header())
    assert [int(it.rgb_off) for it in plan.items] == [int(it.src_off) for it in want.items]
    from pigeon_amd.packing import packed_layout
    assert ([int(it.rgb_off) for it in plan.items], plan.prep.packed_bytes) == packed_layout(sizes)
    # an image the caller supplies has a place in the packed buffer and nothing else
    infos = [ops.jpeg_probe(fx["files"][i]) for i in fx["ok"][:3]]
    infos[1].reason = 2
    p3 = ops.jpeg_plan(infos)
    assert p3.items[1].ncomp == 0 and list(p3.items[1].coef_off) == [0, 0, 0] and p3.items[1].rgb_off == p3.prep.items[1].src_off
    assert p3.items[2].coef_off[0] == p3.items[0].coef_off[0] + sum(p3.items[0].bw[c] * p3.items[0].bh[c] for c in range(3)) * 128


def _patched(data, marker, rel, value):
    """`data` with byte `rel` of the first segment `marker`'s payload replaced."""
    d = bytearray(data)
    pos = 2
    while d[pos + 1] != marker:
        pos += 2 + (d[pos + 2] << 8 | d[pos + 3])
    d[pos + 4 + rel] = value
    return bytes(d)


def _without(data, marker):
    d = bytearray(data)
    pos = 2
    while d[pos + 1] != marker:
        pos += 2 + (d[pos + 2] << 8 | d[pos + 3])
    del d[pos:pos + 2 + (d[pos + 2] << 8 | d[pos + 3])]
    return bytes(d)


def _one_component_scan(data):
    """The SOS segment replaced by one that holds the first component only: a file of several scans."""
    d = bytearray(data)
    pos = 2
    while d[pos + 1] != 0xDA:
        pos += 2 + (d[pos + 2] << 8 | d[pos + 3])
    d[pos:pos + 2 + (d[pos + 2] << 8 | d[pos + 3])] = bytes([0xFF, 0xDA, 0, 8, 1, d[pos + 5], d[pos + 6], 0, 63, 0])
    return bytes(d)


def test_every_refused_kind_comes_back_with_its_reason(fx):
    ops = fx["ops"]
    for i, r in enumerate(fx["refused"]):
        info = ops.jpeg_probe(fx["files"][i])
        assert ops.jpeg_reason(info.reason) == (r or "ok"), fx["names"][i]
        if not r:
            assert (info.height, info.width) == fx["shapes"][i]
    colour = fx["files"][fx["names"].index("17x33_420_smooth_q75")]
    nojfif = _without(colour, 0xE0)
    rgb_ids = _patched(_patched(_patched(nojfif, 0xC0, 6, ord("R")), 0xC0, 9, ord("G")), 0xC0, 12, ord("B"))
    rgb_ids = _patched(_patched(_patched(rgb_ids, 0xDA, 1, ord("R")), 0xDA, 3, ord("G")), 0xDA, 5, ord("B"))
    crafted = {"precision": _patched(colour, 0xC0, 0, 12), "size": _patched(_patched(colour, 0xC0, 1, 0), 0xC0, 2, 0),
               "sampling": _patched(colour, 0xC0, 7, 0x12), "arithmetic": colour.replace(b"\xff\xc0", b"\xff\xc9", 1),
               "lossless": colour.replace(b"\xff\xc0", b"\xff\xc3", 1), "colorspace": rgb_ids, "not_jpeg": b"GIF89a" + bytes(32),
               "malformed": colour[:200], "dnl": colour.replace(b"\xff\xc4", b"\xff\xdc", 1),
               "multiscan": _one_component_scan(colour)}
    assert ops.jpeg_reason(ops.jpeg_probe(nojfif).reason) == "ok"            # ids 1,2,3 without a JFIF marker: YCbCr
    assert ops.jpeg_reason(ops.jpeg_probe(_patched(colour, 0xC0, 7, 0x41)).reason) == "sampling"      # 4:1:1
    too_big = _patched(colour, 0xC0, 1, 0x40)
    assert ops.jpeg_reason(ops.jpeg_probe(_patched(too_big, 0xC0, 2, 1)).reason) == "size"            # height 16385
    for reason, data in crafted.items():
        assert ops.jpeg_reason(ops.jpeg_probe(data).reason) == reason, reason
        with pytest.raises(R.Refused) as e:                            # and the restatement refuses it for the same reason
            R.parse(data)
        assert e.value.reason == reason
    assert "progressive" in ops.jpeg_reason_text(2).lower()


def damaged_cases(fx):
    """Every truncation of two small fixtures and single-byte mutations of their headers: [(what, bytes, size of the original)]."""
    out = []
    for name in ("8x8_420_noise_q75", "9x17_grey_smooth_rst1"):
        i = fx["names"].index(name)
        data, size = fx["files"][i], fx["shapes"][i]
        for n in range(len(data)):
            out.append((f"{name}[:{n}]", data[:n], size))
        scan = R.parse(data)["scan"]
        for p in range(2, scan):
            for x in (0xFF, 0x01, 0x80):
                d = bytearray(data)
                d[p] ^= x
                out.append((f"{name}[{p}]^={x:#x}", bytes(d), None))
    return out


def _decode_one(fx, data):
    """('ok', (h, w)) | ('refused', reason) | ('error', message)"""
    ops = fx["ops"]
    info = ops.jpeg_probe(data)
    if info.reason:
        return "refused", ops.jpeg_reason(info.reason)
    plan = ops.jpeg_plan([info])
    try:
        ops.jpeg_entropy_decode([data], plan, torch.zeros(plan.coef_bytes, dtype=torch.uint8), threads=1)
    except ops.JpegEntropyError as e:
        assert e.index == 0 and "image 0" in str(e)
        return "error", str(e)
    return "ok", (info.height, info.width)


def test_truncations_and_header_mutations_never_succeed_with_another_size(fx):
    try:
        import io
        from PIL import Image
    except ImportError:
        Image = None
    kinds = {"ok": 0, "refused": 0, "error": 0}
    for what, data, size in damaged_cases(fx):
        kind, val = _decode_one(fx, data)
        kinds[kind] += 1
        if size is not None:
            assert kind != "ok", f"{what}: a truncated file decoded"
        elif kind == "ok" and Image is not None:
            try:
                w, h = Image.open(io.BytesIO(data)).size
            except Exception:
                continue                                              # Pillow refuses the file: there is no size to differ from
            assert val == (h, w), f"{what}: {val} but Pillow reports {(h, w)}"
    assert kinds["error"] > 100 and kinds["refused"] > 100, kinds


def test_planted_entropy_errors_name_the_image(fx):
    ops = fx["ops"]
    good = [fx["files"][fx["names"].index(n)] for n in ("8x8_420_noise_q75", "9x17_grey_smooth_rst1", "17x33_444_noise_q75")]
    rst = bytearray(good[1])
    p = rst.index(b"\xff\xd1", R.parse(good[1])["scan"])
    rst[p + 1] = 0xD3                                                  # RST1 -> RST3: out of sequence
    cut = good[2][:R.parse(good[2])["scan"] + 30]                      # the data ends inside an MCU
    noeoi = good[0][:-2]
    for bad, text in ((bytes(rst), "RSTn"), (cut, "inside an MCU"), (noeoi, "EOI")):
        for threads in (1, 16):
            files = [good[0], good[2], bad, good[1]]
            plan = _plan(fx, files)
            with pytest.raises(ops.JpegEntropyError, match=f"image 2.*{text}") as e:
                ops.jpeg_entropy_decode(files, plan, torch.zeros(plan.coef_bytes, dtype=torch.uint8), threads=threads)
            assert e.value.index == 2


def test_wrappers_validate_their_arguments(fx):
    ops, lib = fx["ops"], fx["lib"]
    files = [fx["files"][fx["ok"][0]]]
    plan = _plan(fx, files)
    with pytest.raises(lib.PigeonHipError, match="coefficient buffer"):
        ops.jpeg_entropy_decode(files, plan, torch.zeros(plan.coef_bytes + 1, dtype=torch.uint8))
    with pytest.raises(lib.PigeonHipError, match="files for a plan"):
        ops.jpeg_entropy_decode(files * 2, plan, torch.zeros(plan.coef_bytes, dtype=torch.uint8))
    with pytest.raises(lib.PigeonHipError, match="expects bytes"):
        ops.jpeg_probe("not bytes")
    bad = lib.JpegInfo()
    bad.height, bad.width, bad.ncomp, bad.hs, bad.vs = 8, 8, 3, 1, 2
    with pytest.raises(lib.PigeonHipError, match="image 0"):
        ops.jpeg_plan([bad])
    bad.hs, bad.vs, bad.height = 1, 1, 0
    with pytest.raises(lib.PigeonHipError, match="image 0"):
        ops.jpeg_plan([bad])
    assert 1 <= ops.default_jpeg_threads() <= min(16, len(os.sched_getaffinity(0)))
    assert ops.jpeg_plan([]).coef_bytes == 0


def test_encoded_images_pickle_and_refuse_non_bytes(fx):
    import pickle
    from pigeon_amd.jpeg import EncodedImages
    e = EncodedImages(fx["files"][:3])
    back = pickle.loads(pickle.dumps(e))
    assert back.files == e.files and len(back) == 3 and len(e[1:]) == 2
    assert EncodedImages.concat([e[:1], e[1:]]).files == e.files
    with pytest.raises(TypeError, match="item 1"):
        EncodedImages([b"x", "y"])


def test_standalone_program_under_sanitizers_reports_nothing(fx, tmp_path):
    """The same truncations and mutations through a stand-alone program (its own main, only jpeg_entropy.h) built with the host
    compiler and -fsanitize=address,undefined: no report, and the same verdict per case as the library gives."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_entropy_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           os.path.join(ROOT, "pigeon_amd", "csrc"), os.path.join(ROOT, "tests", "jpeg_entropy_main.cpp"), "-o", exe]
    # (the runtimes linked statically where the compiler has them that way: the program then needs nothing from its environment)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower() or "sanitizer" in build.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    cases = damaged_cases(fx) + [(fx["names"][i], fx["files"][i], None) for i in fx["ok"][::7]]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for _, data, _ in cases:
            f.write(struct.pack("<I", len(data)) + data)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    for (what, data, _), line in zip(cases[::37], lines[::37]):
        kind, _ = _decode_one(fx, data)
        assert line.split()[0] == kind, (what, line)


def test_new_kernels_have_no_scratch_and_no_waterfall_loops(hip_lib):
    """The two kernels index their descriptor through wave-uniform addresses and keep their 8 x 8 in registers and LDS: the ISA of the
    built library shows no scratch and no readfirstlane loop around a descriptor (tools/asm_audit.py, as tests/test_asm_audit.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_audit
    res = {k: v for k, v in asm_audit.audit(os.path.join(ROOT, "pigeon_amd", "libpigeon_hip.so")).items() if "jpeg_" in k}
    assert len(res) == 2 and any("jpeg_idct_kernel" in k for k in res) and any("jpeg_rgb_kernel" in k for k in res), list(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["waterfall"] == 0 and 0 < v["vgpr"] <= 64, (name, v)
