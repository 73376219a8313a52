#!/usr/bin/env python3
"""Generate tests/golden/leanmap.npz: level-0 fixtures of the LEAN-map builders from the REAL reference.

Run in the build container only (needs /root/reference, or the reference's checkout as the first argument):

    python tests/golden/make_leanmap_golden.py [path/to/reference]

What comes from where:
  * normal maps: the reference's own ``dmap2nmap()`` (utils/dmap2nmap.cpp), compiled unchanged.  A small driver written
    below defines ``cimg_display 0`` (no X11), renames the tool's ``main`` and includes the reference's file, so the function
    that runs is the reference's text and the compiler's arithmetic; the binary lives in a temporary directory and is
    never stored.
  * moments: utils/nmap2leanmap.cpp cannot be compiled here (it switches on OpenEXR in CImg and no OpenEXR header is
    installed).  Its per-texel body (l.33-54) is seven float operations with no library call, so ``nmap2leanmap_np`` below
    restates it in numpy float32, one rounding per operation, and that restatement is the source of the moment fixtures.
    The same kind of restatement of dmap2nmap (``dmap2nmap_np``) is checked against the compiled reference on every
    fixture map before anything is written: it must reproduce every byte.

The fixtures are data (inputs and recorded outputs); no reference source is stored.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

DRIVER = r"""
#define cimg_display 0
#define main dmap2nmap_tool_main
#include "%(ref)s/utils/dmap2nmap.cpp"
#undef main
// raw bytes in, raw bytes out: w h scale in_file out_file; images are row-major, x fastest
int main(int argc, char **argv)
{
	if (argc != 6) return 2;
	int w = atoi(argv[1]), h = atoi(argv[2]);
	float scale = (float)atof(argv[3]);
	CImg<uint8_t> dmap(w, h, 1, 1), nmap;
	FILE *f = fopen(argv[4], "rb");
	if (!f) return 3;
	for (int j = 0; j < h; ++j) for (int i = 0; i < w; ++i) dmap(i, j) = (uint8_t)fgetc(f);
	fclose(f);
	dmap2nmap(dmap, nmap, scale);
	f = fopen(argv[5], "wb");
	if (!f) return 4;
	for (int j = 0; j < h; ++j) for (int i = 0; i < w; ++i) for (int c = 0; c < 3; ++c) fputc(nmap(i, j, 0, c), f);
	fclose(f);
	return 0;
}
"""

f32 = np.float32


def dmap2nmap_np(d, scale):
    """utils/dmap2nmap.cpp:20-43 in numpy: float32 operations one at a time, the double steps in float64."""
    h, w = d.shape
    z = d.astype(f32) / f32(255)
    zl, zr = np.concatenate([z[:, :1], z[:, :-1]], 1), np.concatenate([z[:, 1:], z[:, -1:]], 1)      # atXY clamps
    zt, zb = np.concatenate([z[:1], z[:-1]], 0), np.concatenate([z[1:], z[-1:]], 0)
    sx = (f32(w) * f32(0.5)) * f32(scale) * (zr - zl)
    sy = (f32(h) * f32(0.5)) * f32(scale) * (zt - zb)
    nrm_sqr = (f32(1) + sx * sx) + sy * sy
    nrm_inv = (1.0 / np.sqrt(nrm_sqr.astype(np.float64))).astype(f32)
    nx, ny, nz = -sx * nrm_inv, -sy * nrm_inv, nrm_inv
    t1 = (0.5 * nx.astype(np.float64) + 0.5).astype(f32)
    t2 = (0.5 * ny.astype(np.float64) + 0.5).astype(f32)
    return np.stack([(t1 * f32(255)).astype(np.uint8), (t2 * f32(255)).astype(np.uint8), (nz * f32(255)).astype(np.uint8)], 2)


def nmap2leanmap_np(nmap, base_roughness):
    """utils/nmap2leanmap.cpp:33-54 in numpy float32 -> [h, w, 5] = E1..E5 (a blue byte of 0 divides by zero, as there)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (nmap[..., 0].astype(f32) / f32(255)) * f32(2) - f32(1)
        t2 = (nmap[..., 1].astype(f32) / f32(255)) * f32(2) - f32(1)
        t3 = nmap[..., 2].astype(f32) / f32(255)
        sx, sy = -t1 / t3, -t2 / t3
        br = f32(0.5) * f32(base_roughness) * f32(base_roughness)
        return np.stack([sx, sy, sx * sx + br, sy * sy + br, sx * sy], 2).astype(f32)


def height_maps():
    """seeded height maps [h, w]: white noise (steep), and a smooth bumpy one (the map the variance tests use)"""
    rng = np.random.default_rng(20100221)
    maps = {}
    for name, (w, h) in {"n64x32": (64, 32), "n1x1": (1, 1), "n2x1": (2, 1), "n1x4": (1, 4)}.items():
        maps[name] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    y, x = np.mgrid[0:128, 0:128].astype(np.float64) / 128.0
    bumps = 0.5 + 0.2 * np.sin(2 * np.pi * 3 * x) * np.cos(2 * np.pi * 2 * y) + 0.15 * np.sin(2 * np.pi * (7 * x + 5 * y)) \
        + 0.1 * rng.random((128, 128))
    maps["b128x128"] = np.clip(bumps * 255.0, 0, 255).astype(np.uint8)
    return maps


def main():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER % {"ref": REF})
        subprocess.run(["g++", "-O2", "-w", src, "-o", exe, "-lpthread"], check=True)
        out = {}
        for name, d in height_maps().items():
            h, w = d.shape
            out[f"dmap_{name}"] = d
            for tag, scale in (("s01", 0.1), ("s4", 4.0)):
                fi, fo = os.path.join(tmp, "in.raw"), os.path.join(tmp, "out.raw")
                d.tofile(fi)
                subprocess.run([exe, str(w), str(h), repr(scale), fi, fo], check=True)
                nmap = np.fromfile(fo, np.uint8).reshape(h, w, 3)
                assert np.array_equal(nmap, dmap2nmap_np(d, scale)), f"the numpy restatement of dmap2nmap differs from the reference on {name} / {scale}"
                out[f"nmap_{name}_{tag}"] = nmap
                if tag == "s01" and name != "b128x128":     # 128 x 128 x 5 floats would be most of the file: the tests restate it from the stored normal map
                    out[f"lean_{name}_{tag}"] = nmap2leanmap_np(nmap, 1e-5)
        # a normal map the tools would never make but a caller may hand in: blue bytes of 0 and 1 (infinite / huge slopes, 0 / 0)
        rng = np.random.default_rng(7)
        hostile = rng.integers(0, 256, (4, 8, 3), dtype=np.uint8)
        hostile[0, 0, 2] = 0; hostile[1, 3] = (128, 127, 0); hostile[2, 5, 2] = 1; hostile[3, 7] = (255, 0, 0)
        out["nmap_hostile"] = hostile
        out["lean_hostile"] = nmap2leanmap_np(hostile, 0.05)
        out["scales"] = np.array([0.1, 4.0], np.float32)
    path = os.path.join(HERE, "leanmap.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", ", ".join(f"{k}{v.shape}" for k, v in out.items()))
    print("smallest blue byte of the bumpy map:", out["nmap_b128x128_s01"][..., 2].min(), "at scale 0.1,", out["nmap_b128x128_s4"][..., 2].min(), "at scale 4")


if __name__ == "__main__":
    main()
