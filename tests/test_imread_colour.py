"""facade::imread (host/slam_facade.h) with IMREAD_COLOR and, unchanged, IMREAD_GRAYSCALE: a stand-alone program
(tests/cpp/imread_colour_main.cpp, its own main, no GPU, no library of the project) reads PNGs of every colour type the reader
takes — rows filtered by hand with each of PNG's filter types — and a PGM, and must give what numpy gives.  Damaged files
(every truncation at a stride of 7 bytes, each of the first 40 bytes flipped) must give an empty image or one of the header's
size.  The program is built twice, plain and with the host sanitizers (address, undefined), and run as a child process."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_colour as rc
from colour_cases import write_png as _png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREY, COLOR = 0, 1


def _build(d, sanitize):
    exe = str(d / ("imread_colour_asan" if sanitize else "imread_colour"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include")]
    if sanitize:
        # the sanitizer's runtime is linked into the program itself: the child needs nothing preloaded
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "imread_colour_main.cpp"), "-o", exe, "-lz"])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("imread_colour")
    return [_build(d, False), _build(d, True)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, r g b uint8 [h, w, 3] as the file holds it)"""
    d = tmp_path_factory.mktemp("imread_files")
    rng = np.random.default_rng(17)
    h, w = 11, 23
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgb[0, 0] = (255, 0, 0); rgb[0, 1] = (0, 255, 0); rgb[0, 2] = (0, 0, 255); rgb[0, 3] = (255, 255, 255); rgb[0, 4] = (0, 0, 0)
    alpha = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
    out = {}
    every = (0, 1, 2, 3, 4)
    for name, arr, filters, as_rgb in (("rgb", rgb, every, rgb), ("rgb_plain", rgb, (0,), rgb), ("rgba", np.concatenate([rgb, alpha], 2), every, rgb),
                                       ("grey", grey, every, np.repeat(grey[:, :, None], 3, 2)),
                                       ("grey_alpha", np.concatenate([grey[:, :, None], alpha], 2), (4, 3, 2, 1), np.repeat(grey[:, :, None], 3, 2))):
        p = str(d / (name + ".png"))
        _png(p, arr, filters)
        out[name] = (p, as_rgb)
    p = str(d / "grey.pgm")
    with open(p, "wb") as f:
        f.write(b"P5\n# a comment\n%d %d\n255\n" % (w, h) + grey.tobytes())
    out["pgm"] = (p, np.repeat(grey[:, :, None], 3, 2))
    return out


def _dump(exe, flags, path, tmp):
    r = subprocess.run([exe, "dump", str(flags), path, tmp], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    cols, rows, ch = (int(v) for v in r.stdout.split())
    data = np.fromfile(tmp, np.uint8)
    return cols, rows, ch, data


def test_colour_and_grey_reads_equal_numpy(programs, files, tmp_path):
    tmp = str(tmp_path / "out.bin")
    for exe in programs:
        for name, (path, rgb) in files.items():
            h, w, _ = rgb.shape
            cols, rows, ch, data = _dump(exe, COLOR, path, tmp)
            assert (cols, rows, ch) == (w, h, 3), (exe, name)
            assert np.array_equal(data.reshape(h, w, 3), rgb[:, :, ::-1]), (exe, name)          # b, g, r
            # IMREAD_GRAYSCALE: what the reader gave before it knew colour — the grey byte of a grey file, the weighted sum of a colour one
            cols, rows, ch, data = _dump(exe, GREY, path, tmp)
            assert (cols, rows, ch) == (w, h, 1), (exe, name)
            want = rgb[:, :, 0] if name in ("grey", "grey_alpha", "pgm") else rc.grey_from_bgr(rgb[:, :, ::-1])
            assert np.array_equal(data.reshape(h, w), want), (exe, name)
    # the primaries written into the first pixels
    assert [int(v) for v in rc.grey_from_bgr(files["rgb"][1][:1, :5, ::-1])[0]] == [76, 150, 29, 255, 0]


def test_a_file_that_cannot_be_read_is_an_empty_image(programs, tmp_path):
    tmp = str(tmp_path / "out.bin")
    junk = str(tmp_path / "junk.png")
    open(junk, "wb").write(b"not an image at all, whatever its name says")
    for exe in programs:
        for path in (junk, str(tmp_path / "missing.png")):
            for flags in (GREY, COLOR):
                assert _dump(exe, flags, path, tmp)[:3] == (0, 0, 0)
                assert _dump(exe, flags, path, tmp)[3].size == 0


def test_damaged_colour_files_give_an_empty_image_or_one_of_the_headers_size(programs, files, tmp_path):
    path = files["rgb"][0]
    raw = open(path, "rb").read()
    tmp = str(tmp_path / "mutant.png")
    for exe in programs:
        r = subprocess.run([exe, "fuzz", str(COLOR), path, tmp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        lines = [l.split() for l in r.stdout.splitlines()]
        trunc = [l for l in lines if l[0] == "t"]
        flips = [l for l in lines if l[0] == "f"]
        assert [int(l[1]) for l in trunc] == list(range(0, len(raw), 7)) and [int(l[1]) for l in flips] == list(range(40))
        sized = 0
        for kind, n, cols, rows, ch, size in lines:
            n, cols, rows, ch, size = int(n), int(cols), int(rows), int(ch), int(size)
            if size == 0:
                assert (cols, rows, ch) == (0, 0, 0)
                continue
            mutant = bytearray(raw[:n]) if kind == "t" else bytearray(raw)
            if kind == "f":
                mutant[n] ^= 0xff
            hw, hh = struct.unpack(">II", bytes(mutant[16:24]))
            assert (cols, rows, ch, size) == (hw, hh, 3, hw * hh * 3), (kind, n)
            sized += 1
        # the reader checks no CRC: a file cut inside its last chunks, or flipped in a length it does not use, still reads
        assert 0 < sized < len(lines)
