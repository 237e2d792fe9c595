"""Writes tests/golden/jpeg_fixtures.npz: JPEG files as bytes plus Pillow's `Image.open(f).convert('RGB')` pixels, so that no GPU test
needs Pillow.  `python tests/make_jpeg_fixtures.py`.  Deterministic for one Pillow / libjpeg-turbo build; the pixels committed are
Pillow 12.2.0's.

The sizes are the smallest that reach chroma widths of 1, 2 (replicated, not filtered), 3 (the first filtered width) and more, odd
sizes cropped out of the MCU padding, one MCU, one MCU plus a pixel, and planes of one row / one column.  The quality axis is trimmed
before the size axis: every size in every mode at quality 75 with both contents, qualities 1 and 100 with noise only."""
import io
import os

import numpy as np
from PIL import Image

SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (4, 5), (1, 6), (2, 7), (7, 9), (8, 8), (9, 17), (16, 16), (17, 33), (33, 1), (37, 53)]
MODES = {"grey": None, "444": 0, "422": 1, "420": 2}
VARIANT_SIZES = [(9, 17), (17, 33), (37, 53)]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_fixtures.npz")


def content(kind, h, w, rng):
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 127.5 + 127.5 * np.sin(x / 5.0 + y / 11.0)
    g = 255.0 * (x + 1) / (w + 1)
    b = 255.0 * (y + 1) / (h + 1) * (0.5 + 0.5 * np.cos(x / 3.0))
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def encode(arr, mode, **kw):
    im = Image.fromarray(arr)
    if mode == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = MODES[mode]
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def grid(rng, sizes=SIZES, variant_sizes=VARIANT_SIZES):
    """[(name, file bytes, expected refusal reason or '')]"""
    out = []
    for h, w in sizes:
        for mode in MODES:
            for kind in ("noise", "smooth"):
                for q in ((1, 75, 100) if kind == "noise" else (75,)):
                    out.append((f"{h}x{w}_{mode}_{kind}_q{q}", encode(content(kind, h, w, rng), mode, quality=q), ""))
    for h, w in variant_sizes:
        for mode in MODES:
            for kind in ("noise", "smooth"):
                a = content(kind, h, w, rng)
                variants = {"opt": dict(quality=75, optimize=True), "opt100": dict(quality=100, optimize=True),
                            "rst1": dict(quality=75, restart_marker_blocks=1), "rstrow": dict(quality=75, restart_marker_rows=1),
                            "q255": dict(qtables=[[255] * 64, [255] * 64])}
                for vname, kw in variants.items():
                    try:
                        out.append((f"{h}x{w}_{mode}_{kind}_{vname}", encode(a, mode, **kw), ""))
                    except OSError:                                # Pillow's encoder fails on some noise with optimize=True ("broken data stream")
                        pass
    a = content("smooth", 17, 33, rng)
    out.append(("17x33_progressive", encode(a, "420", quality=75, progressive=True), "progressive"))
    buf = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(buf, "JPEG", quality=75)
    out.append(("17x33_cmyk", buf.getvalue(), "components"))
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "PNG")
    out.append(("17x33_png", buf.getvalue(), "not_jpeg"))
    return out


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    items = grid(np.random.default_rng(20260101))
    files = [np.frombuffer(f, dtype=np.uint8) for _, f, _ in items]
    pixels = [pillow_pixels(f) for _, f, _ in items]
    np.savez_compressed(OUT, names=np.array([n for n, _, _ in items]), refused=np.array([r for _, _, r in items]),
                        files=np.concatenate(files), file_off=np.cumsum([0] + [len(f) for f in files]).astype(np.int64),
                        pixels=np.concatenate([p.reshape(-1) for p in pixels]),
                        shapes=np.array([p.shape[:2] for p in pixels], dtype=np.int32))
    print(f"{len(items)} files, {sum(len(f) for f in files)} file bytes, {sum(p.size for p in pixels)} pixel bytes -> "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
