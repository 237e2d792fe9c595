"""The numpy restatement of the JPEG decoder (tests/_jpegref.py) against Pillow: the pixels committed in tests/golden/jpeg_fixtures.npz,
a freshly generated grid where Pillow is importable, and seven planted mistakes that each have to show -- so that the restatement the
host stage and the kernels are held against is itself pinned, formula by formula."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jpegref as R  # noqa: E402


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    z = np.load(os.path.join(golden_dir, "jpeg_fixtures.npz"))
    off, shapes = z["file_off"], z["shapes"]
    po = np.cumsum([0] + [int(h) * int(w) * 3 for h, w in shapes])
    return [(str(z["names"][i]), z["files"][off[i]:off[i + 1]].tobytes(),
             z["pixels"][po[i]:po[i + 1]].reshape(int(shapes[i][0]), int(shapes[i][1]), 3), str(z["refused"][i])) for i in range(len(shapes))]


def test_fixture_file_covers_the_grid(fixtures):
    names = {n for n, _, _, _ in fixtures}
    for size in ("1x1", "1x2", "2x1", "3x3", "4x5", "1x6", "2x7", "7x9", "8x8", "9x17", "16x16", "17x33", "33x1", "37x53"):
        for mode in ("grey", "444", "422", "420"):
            assert {f"{size}_{mode}_noise_q{q}" for q in (1, 75, 100)} <= names and f"{size}_{mode}_smooth_q75" in names
    for variant in ("opt", "rst1", "rstrow", "q255"):
        assert any(n.endswith("_" + variant) for n in names), variant
    assert sorted(r for _, _, _, r in fixtures if r) == ["components", "not_jpeg", "progressive"]
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_fixtures.npz")) < 512 * 1024


def test_restatement_equals_the_committed_pillow_pixels(fixtures):
    for name, data, want, refused in fixtures:
        if refused:
            with pytest.raises(R.Refused) as e:
                R.decode(data)
            assert e.value.reason == refused, name
            continue
        got = R.decode(data)
        assert got.dtype == np.uint8 and R.first_mismatch(got, want) is None, f"{name}: {R.first_mismatch(got, want)}"


def test_restatement_equals_pillow_on_a_fresh_grid():
    """Other sizes and other content than the committed file, encoded and decoded by the Pillow at hand."""
    pytest.importorskip("PIL")
    import make_jpeg_fixtures as gen
    rng = np.random.default_rng(99)
    sizes = [(5, 3), (3, 4), (15, 31), (24, 40), (41, 23), (64, 6)]
    n = 0
    for name, data, refused in gen.grid(rng, sizes=sizes, variant_sizes=[(24, 40), (41, 23)]):
        if refused:
            continue
        got, want = R.decode(data), gen.pillow_pixels(data)
        assert R.first_mismatch(got, want) is None, f"{name}: {R.first_mismatch(got, want)}"
        n += 1
    assert n > 100


# mistake -> the fixtures on which it has to show: (predicate on the name, why)
PLANTED = {
    "bias_swap": lambda n: "_420_" in n and n.split("_")[0] in ("7x9", "9x17", "16x16", "17x33", "37x53"),
    "filter_at_2": lambda n: ("_420_" in n or "_422_" in n) and n.split("_")[0] == "3x3",                  # the one size with a chroma width of 2
    "pass_swap": lambda n: n.split("_")[0] in ("16x16", "17x33", "37x53") and "noise" in n,
    "no_32768": lambda n: "grey" not in n,
    "zigzag_T": lambda n: n.split("_")[0] in ("16x16", "17x33", "37x53") and "noise" in n,
    "no_dc_reset": lambda n: n.endswith("_rst1") or n.endswith("_rstrow"),
    # an even height whose last chroma row is not the last row of the block grid, and a filtered width: 2x7 (ch 1), 4x5 (2), 8x8 (4)
    "pad_bottom": lambda n: "_420_" in n and n.split("_")[0] in ("2x7", "4x5", "8x8"),
}


@pytest.mark.parametrize("mistake", list(PLANTED))
def test_planted_mistake_is_rejected_with_the_place_named(fixtures, mistake):
    """Each mistake changes pixels on the fixtures made to catch it (and the report names fixture, pixel and channel); on no fixture
    outside the mistake's reach does it change anything it should not."""
    shows = []
    for name, data, want, refused in fixtures:
        if refused or not PLANTED[mistake](name):
            continue
        place = R.first_mismatch(R.decode(data, mistakes={mistake}), want)
        if place is not None:
            shows.append(f"{name}: {place}")
    assert shows, f"{mistake}: no fixture shows it"
    assert all(" y=" in s and " x=" in s and "channel=" in s for s in shows)
    if mistake == "filter_at_2":
        assert any("_420_" in s for s in shows) and any("_422_" in s for s in shows)
    if mistake == "no_dc_reset":
        # nothing but files with restart markers can show it
        for name, data, want, refused in fixtures[::9]:
            if not refused and "_rst" not in name:
                assert R.first_mismatch(R.decode(data, mistakes={mistake}), want) is None, name


def test_restatement_raises_on_a_damaged_scan(fixtures):
    name, data, _, _ = next(f for f in fixtures if f[0] == "17x33_420_noise_q75")
    scan = R.parse(data)["scan"]
    with pytest.raises(R.EntropyError):
        R.decode(data[:scan + 25])
    with pytest.raises(R.EntropyError):
        R.decode(data[:-2])
