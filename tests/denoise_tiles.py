"""tests/denoise_tiles.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Pure-Python model of the launch geometry of the a-trous iteration kernels, hrt_denoise_iter_kernel (csrc/hrt_denoise.hip, shape 1) and
hrt_denoise_temporal_iter_kernel (csrc/hrt_denoise_temporal.hip).  It MIRRORS those kernels and their launch_iter and must move with
them: the 32x8 tile, the halo of 2, the tap step 1 << i, the s * s sub-lattices of pass i, the grid sized for the largest
sub-lattice, and the whole-workgroup return `if (bx >= nx || by >= ny) return;` ahead of the barrier.

Along one axis of length L (W with a tile of 32, H with a tile of 8) pass i with step s = 1 << i has s sub-lattices; the one at offset
o holds n(o) = ceil((L - o) / s) pixels (0 when o >= L) and needs ceil(n(o) / tile) tiles, while the grid gives every sub-lattice
ceil(ceil(L / s) / tile) of them.  What a call exercises along that axis at that step:

  seam            some sub-lattice spans at least 2 tiles: a tile reads halo records that belong to its neighbour tile
  short_lattice   a non-empty sub-lattice needs fewer tiles than the grid holds: its last workgroup returns as a whole with n > 0
  empty_lattice   a sub-lattice holds no pixel (o >= L): every one of its workgroups returns as a whole
  ragged_tile     the last tile of some sub-lattice is partly filled: lanes return after the barrier, halo records lie outside
"""
TILE_W, TILE_H, HALO = 32, 8, 2
TILE = {"x": TILE_W, "y": TILE_H}
KINDS = ("seam", "short_lattice", "empty_lattice", "ragged_tile")


def ceil_div(a, b):
    return -(-a // b)


def lattice_len(length, o, s):
    """Pixels of the sub-lattice at offset o along an axis of `length` pixels: the kernels' (L - o + s - 1) / s, 0 for o >= L."""
    return max(0, ceil_div(length - o, s))


def grid(W, H, s):
    """launch_iter's grid for step s."""
    mx, my = ceil_div(W, s), ceil_div(H, s)
    return ceil_div(mx, TILE_W), ceil_div(my, TILE_H), s * s


def axis_kinds(length, tile, s):
    kinds = set()
    launched = ceil_div(ceil_div(length, s), tile)
    for o in range(s):
        n = lattice_len(length, o, s)
        if n == 0:
            kinds.add("empty_lattice")
            continue
        if ceil_div(n, tile) >= 2:
            kinds.add("seam")
        if ceil_div(n, tile) < launched:
            kinds.add("short_lattice")
        if n % tile:
            kinds.add("ragged_tile")
    return kinds


def classes(W, H, iterations=5):
    """The set of (step, axis, kind) a denoiser call on a W x H image with `iterations` passes exercises."""
    out = set()
    for i in range(iterations):
        s = 1 << i
        for axis, length in (("x", W), ("y", H)):
            out |= {(s, axis, k) for k in axis_kinds(length, TILE[axis], s)}
    return out


def seam_steps(W, H, iterations=5):
    """{step: set of axes} where the call claims `seam`."""
    out = {}
    for s, axis, kind in classes(W, H, iterations):
        if kind == "seam":
            out.setdefault(s, set()).add(axis)
    return out


# The cases of tests/test_denoise_sizes_gpu.py: (width, height, iterations).  hrt_denoise runs CASES; hrt_denoise_temporal, whose
# restatement costs more, runs them without 4097 x 1025: the thin pair covers its steps 32, 64 and 128, one axis each (and, being
# narrower than those steps along the other axis, the empty sub-lattices).
BIG = (4097, 1025, 8)
CASES = [(129, 33, 5), (517, 133, 5), (4097, 24, 8), (40, 1025, 8), BIG]
TEMPORAL_CASES = [c for c in CASES if c != BIG]

# every size the device tests of the two denoisers used before tests/test_denoise_sizes_gpu.py, with the largest iteration count it ran at
OLD_SIZES = [(97, 61, 8), (200, 125, 5), (20, 12, 5), (1, 1, 5), (33, 9, 5), (64, 40, 5), (70, 45, 5), (72, 44, 5), (80, 52, 5),
             (96, 64, 5), (60, 38, 5), (48, 30, 5), (56, 34, 5)]


def union(cases):
    out = set()
    for w, h, it in cases:
        out |= classes(w, h, it)
    return out
