"""Generates tests/golden/jpeg_device/*.jpg for the device JPEG decoder (tests/test_jpeg_device_*.py) and the pixels an independent
libjpeg build (Pillow: libjpeg-turbo with its defaults) decodes from them, as binary PPM / PGM; also index.txt, the table of what the
headers of all 18 fixtures (these nine and the nine of tests/golden/jpeg/) say, read here by a few lines of Python of its own.
Needs Pillow; the fixtures are committed so that the tests run anywhere.

    python tests/golden/make_jpeg_device_fixtures.py

The cases are about restart intervals (the device entropy stage runs one lane per interval): many of them, ragged last ones, none,
DRI without a marker in the stream, custom tables, and the tiny sizes at which the chroma filters fall back to replication.
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg_device")
OLD = os.path.join(HERE, "jpeg")
os.makedirs(OUT, exist_ok=True)


def scene(h, w, seed):
    """the scene() of make_jpeg_fixtures.py (that script writes its files when imported, so the function is restated)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 120 * np.sin(x / 7.0 + y / 13.0), 127 + 120 * np.cos(x / 5.0 - y / 9.0), 255.0 * ((x // 6 + y // 4) % 2)], 2)
    img += rng.normal(0, 25, img.shape)
    img[h // 3: h // 3 + 5, :, :] = (250, 10, 30)
    return np.clip(img, 0, 255).astype(np.uint8)


def headers(data):
    """(rows, cols, channels, restart interval, intervals) from SOF0 / DRI"""
    i, dri, sof = 2, 0, None
    while i + 4 <= len(data):
        m = data[i + 1]; L = (data[i + 2] << 8) | data[i + 3]
        s = data[i + 4:i + 2 + L]
        if m in (0xC0, 0xC1):
            sof = s
        elif m == 0xDD:
            dri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            break
        i += 2 + L
    h, w, nc = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    hs = [sof[7 + 3 * c] >> 4 for c in range(nc)]; vs = [sof[7 + 3 * c] & 15 for c in range(nc)]
    hmax, vmax = (max(hs), max(vs)) if nc > 1 else (1, 1)
    mcus = -(-w // (8 * hmax)) * -(-h // (8 * vmax))
    return h, w, nc, dri, (-(-mcus // dri) if dri else 1)


CASES = [  # name, size (h, w), mode, save options
    ("d420_dri1", (120, 168), "RGB", dict(quality=85, subsampling=2, restart_marker_blocks=1)),        # 88 intervals
    ("d420_dri5_odd", (131, 203), "RGB", dict(quality=92, subsampling=2, restart_marker_blocks=5)),    # short last interval, odd size
    ("d444_dri2", (41, 67), "RGB", dict(quality=90, subsampling=0, restart_marker_blocks=2)),
    ("d422_dri1_opt", (40, 150), "RGB", dict(quality=75, subsampling=1, restart_marker_blocks=1, optimize=True)),      # custom tables
    ("dgray_dri4", (70, 93), "L", dict(quality=80, restart_marker_blocks=4)),
    ("d420_tiny", (3, 4), "RGB", dict(quality=90, subsampling=2)),                                      # cw = 2: replication
    ("d422_tiny_dri1", (9, 3), "RGB", dict(quality=90, subsampling=1, restart_marker_blocks=1)),
    ("d420_q100", (48, 64), "RGB", dict(quality=100, subsampling=2, restart_marker_rows=1)),
    ("d420_one_interval", (32, 48), "RGB", dict(quality=80, subsampling=2, restart_marker_blocks=100)),  # DRI, no marker in the stream
]
if __name__ == "__main__":
    for k, (name, (h, w), mode, opts) in enumerate(CASES):
        a = scene(h, w, 200 + k)
        im = Image.fromarray(a).convert(mode)
        path = os.path.join(OUT, name + ".jpg")
        im.save(path, "JPEG", **opts)
        dec = Image.open(path)
        dec.load()
        dec.save(os.path.join(OUT, name + (".pgm" if mode == "L" else ".ppm")))
    with open(os.path.join(OUT, "index.txt"), "w") as f:
        f.write("# name rows cols channels restart_interval intervals\n")
        for d in (OLD, OUT):
            for fn in sorted(os.listdir(d)):
                if fn.endswith(".jpg") and "progressive" not in fn:
                    line = "%s %d %d %d %d %d" % ((fn[:-4],) + headers(open(os.path.join(d, fn), "rb").read()))
                    print(line, os.path.getsize(os.path.join(d, fn)), "bytes")
                    f.write(line + "\n")
