"""fp64 reference, elementwise error bound, input families, operand layouts and a plain model (with its wrong turns) of the
weight-gradient GEMM out = X^T Y on K-major bf16 operands (csrc/gemm_tn.hip), shared by test_gemm_tn_bound.py (no GPU) and
test_gpu_gemm_tn_elementwise.py, in the style of gemm_epi_ref.py (G and worst_ratio come from there).

The bound.  Split s of S sums K_s of the K products.  A product of two bf16 values has 16 significant bits and is exact in fp32;
n such terms summed in fp32 in ANY order (the MFMA's order inside 16 k-rows, then accumulator += per 16 k-rows) are off by at
most gamma_{n-1} sum |terms| with gamma_n = n G / (1 - n G) [Higham, Accuracy and Stability, sec. 4.2], and gamma_{n-1} <= n G
while n (n - 1) G <= 1, i.e. n <= 4096:  |p_s - P_s| <= K_s G A_s, A_s the split's share of absacc = |X|^T |Y|.  The reduce adds
the S partials in index order, S - 1 roundings of a running sum that is never above sum_s |p_s| <= (1 + K G) absacc:
<= (S - 1) G (1 + K G) absacc <= S G absacc.  Together
    |out - want64| <= max_s K_s G absacc + S G absacc <= (K + S) G absacc          (`bound`; + 1e-30 for absacc = 0).
This is gemm_epi_ref.acc_bound (K products + the bias add) with the S - 1 adds of the reduce in place of the bias add.  Nothing
in it is fitted.

The families.  `real`: gpu_util.asym rounded to bf16 (asymmetric, sign-varying).  `exact`: hash-derived integers in
{+-1, +-2, +-3, +-4}, never zero.  Every product is an integer of magnitude <= 16 and absacc <= 16 K = 4 688 < 2^14 at the
largest K below, far under 2^24, so every partial sum in any order is an integer fp32 holds exactly: a right kernel equals the
fp64 reference BIT FOR BIT, whatever its tile, ring depth or split count, and because no operand is zero every dropped, doubled
or misplaced product moves an element.

The layouts (`layout`).  Every operand is a [K, width] window of a larger buffer: GUARD_BEFORE rows above, GUARD_AFTER rows
below, ld >= width, a column offset that keeps the window 16-byte aligned.  `tight` is ld == width; `proj_out` is the model's
proj_out_weight call (Y of width d at column d of a [K, 2d] buffer, X tight), `proj_in` its proj_in_weight call (Y at column 0
of the same buffer), with X padded there; `padded` is ld = width + 8 j with an offset on both.

`emulate` is the arithmetic of all three kernels as plain torch: fp32, 16 k-rows per step, K-tiles of k_tile rows dealt to the
splits as the kernels do (per = ceil(nkt / S) tiles each, trailing splits empty), rows past K zero, partials added in index
order.  `mutate` is `emulate` with one wrong turn a pipelined K-major GEMM can take (MUTATIONS).  test_gemm_tn_bound.py shows
that the bound admits `emulate` with room (<= 0.25) and refuses every mutation (> 2.0, bit-unequal on `exact`) wherever the
mutation changes anything: the GPU test's `<= 1.0` and `torch.equal` therefore tell a right kernel from each of these.
"""
import functools

import torch

from gemm_epi_ref import G, worst_ratio  # noqa: F401  (re-exported: the two tests take them from here)

SHAPES = [(8, 8), (8, 264), (136, 120), (264, 392)]                      # (Mo, No)
KS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 161, 192, 193, 293]
SPLITS = [1, 2, 3, 4, 7]
FAMILIES = ["real", "exact"]
LAYOUTS = ["tight", "proj_out", "padded", "proj_in"]
GUARD_BEFORE, GUARD_AFTER = 2, 3
# every (K, k_splits, layout) both tests run, at every shape, family and kernel: each K meets all four layouts, each split count too
CASES = [(K, S, LAYOUTS[(ik + js) % len(LAYOUTS)]) for ik, K in enumerate(KS) for js, S in enumerate(SPLITS)]
MUTATIONS = ["drop_row", "row_K", "drop_last_tile", "tile_twice", "stale_stage", "swizzle", "ld_as_width", "swap_xy"]
_POOL = (max(KS) + GUARD_BEFORE + GUARD_AFTER, 2 * max(n for _, n in SHAPES))


def layout(name, Mo, No):
    """(ldx, X column offset, ldy, Y column offset) in elements"""
    return {"tight": (Mo, 0, No, 0), "proj_out": (Mo, 0, 2 * No, No), "padded": (Mo + 8, 8, No + 24, 16),
            "proj_in": (Mo + 16, 0, 2 * No, 0)}[name]


@functools.lru_cache(maxsize=None)
def pool(family, seed):
    """bf16 [_POOL]: every operand and every finite fill is a top-left slice of one of these (a pure function of family, seed)"""
    if family == "real":
        from gpu_util import asym
        return asym(_POOL, seed).to(torch.bfloat16)
    from ditto_tts_amd.synth import hash_uniform
    u = torch.from_numpy(hash_uniform(_POOL, "tn_exact", seed))
    mag = (4 * u.abs()).floor().clamp(max=3) + 1
    return torch.where(u < 0, -mag, mag).to(torch.bfloat16)


def place(data, ld, off, fill):
    """data [K, width] -> (buffer [GUARD_BEFORE + K + GUARD_AFTER, ld], view of the window's columns from its row 0 to the
    buffer's last row: rows >= K of the view are guard rows).  fill: a float (NaN) or a tensor at least as large as the buffer,
    whose values surround the window."""
    K, width = data.shape
    rows = GUARD_BEFORE + K + GUARD_AFTER
    assert off % 8 == 0 and ld % 8 == 0 and off + width <= ld
    if isinstance(fill, torch.Tensor):
        buf = fill[:rows, :ld].clone()
    else:
        buf = torch.full((rows, ld), fill, dtype=data.dtype, device=data.device)
    buf[GUARD_BEFORE:GUARD_BEFORE + K, off:off + width] = data
    return buf, buf[GUARD_BEFORE:, off:off + width]


def operands(family, Mo, No, K, lay, finite_fill=False, device="cpu", pools=pool):
    """(X buffer, X view, ldx, Y buffer, Y view, ldy): seeds 31 / 32 as test_weight_gradient_gemm_tn; what surrounds the windows
    is NaN, or with finite_fill other values of the same family (what a wrong read finds in the model's buffers)"""
    ldx, ox, ldy, oy = layout(lay, Mo, No)
    px, py = pools(family, 31), pools(family, 32)
    fx, fy = (pools(family, 33), pools(family, 34)) if finite_fill else (float("nan"), float("nan"))
    if device != "cpu":
        px, py = px.to(device), py.to(device)
    xb, xv = place(px[:K, :Mo], ldx, ox, fx)
    yb, yv = place(py[:K, :No], ldy, oy, fy)
    return xb, xv, ldx, yb, yv, ldy


def reference(X, Y):
    """X [K, Mo], Y [K, No] bf16 (the windows) -> want64 = X^T Y in fp64 and absacc = |X|^T |Y|"""
    x, y = X.double(), Y.double()
    return x.T @ y, x.abs().T @ y.abs()


def bound(absacc, K, S):
    return (K + max(S, 1)) * G * absacc + 1e-30


# ------------------------------------------------------------ the model ------------------------------------------------------------
def split_tiles(K, S, k_tile):
    """the K-tile indices of every split: per = ceil(nkt / S) each, the last non-empty one takes what is left, the rest none"""
    nkt, S = -(-K // k_tile), max(S, 1)
    per = -(-nkt // S)
    return [list(range(s * per, min(nkt, (s + 1) * per))) for s in range(S)]


def _rows(V, K, k0, which=None):
    """fp32 [16, width]: rows k0 .. k0 + 15 of the operand, the zero row for every row index >= K"""
    out = torch.zeros(16, V.shape[1], dtype=torch.float32, device=V.device)
    hi = min(K, k0 + 16)
    if hi > k0:
        out[:hi - k0] = V[k0:hi].float()
    return out


def _accumulate(X, Y, K, tiles, k_tile, fetch=_rows, step=None):
    parts = []
    for s, ts in enumerate(tiles):
        acc = torch.zeros(X.shape[1], Y.shape[1], dtype=torch.float32, device=X.device)
        for i, t in enumerate(ts):
            for h in range(k_tile // 16):
                xs, ys = fetch(X, K, t * k_tile + 16 * h, "x"), fetch(Y, K, t * k_tile + 16 * h, "y")
                c = xs.T @ ys
                if step is not None:
                    c = step(s, i, h, xs, ys, c)
                acc = acc + c
        parts.append(acc)
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def emulate(X, Y, K, S, k_tile):
    """X, Y: 2-D bf16 views with at least K rows (`place`'s views; rows >= K are never read) -> fp32 [Mo, No]"""
    return _accumulate(X, Y, K, split_tiles(K, S, k_tile), k_tile)


def mutate(name, X, Y, K, S, k_tile):
    """`emulate` with one wrong turn.  X, Y as `place` returns them: the rows below K and the columns beside the window are there
    to be read by the turns that read them."""
    tiles = split_tiles(K, S, k_tile)
    fetch, step = _rows, None
    if name == "drop_row":            # k-row K // 2 never arrives (both operands: its products are missing)
        def fetch(V, K_, k0, which):
            r = _rows(V, K_, k0)
            if k0 <= K // 2 < k0 + 16:
                r[K // 2 - k0] = 0
            return r
    elif name == "row_K":             # `k <= K` for `k < K`: the row under the window instead of the zero row
        def fetch(V, K_, k0, which):
            r = _rows(V, K_, k0)
            if k0 <= K < k0 + 16:
                r[K - k0] = V[K].float()
            return r
    elif name == "drop_last_tile":    # the last split that has tiles stops one short
        last = max(s for s, ts in enumerate(tiles) if ts)
        tiles[last] = tiles[last][:-1]
    elif name == "tile_twice":        # split 0 runs one tile into split 1's range
        if len(tiles) > 1 and tiles[1]:
            tiles[0] = tiles[0] + tiles[1][:1]
    elif name == "stale_stage":       # split 0, its fifth tile (the first to re-use a ring stage), second half-step, the wave block
        def step(s, i, h, xs, ys, c):  # of output rows and columns 0..63: the fragments are those of four tiles earlier
            if s == 0 and i == 4 and h == 1:
                k0 = tiles[0][0] * k_tile + 16
                old = _rows(X, K, k0).T @ _rows(Y, K, k0)
                c = c.clone()
                c[:64, :64] = old[:64, :64]
            return c
    elif name == "swizzle":           # chunks 0 and 1 (8 columns each) of Y's row 0 land in each other's place
        def fetch(V, K_, k0, which):
            r = _rows(V, K_, k0)
            if which == "y" and k0 == 0 and r.shape[1] >= 16:
                r[0, :16] = torch.cat([r[0, 8:16], r[0, :8]])
            return r
    elif name == "ld_as_width":       # row k at k * width instead of k * ld: Y where it has a stride of its own, else X
        if Y.stride(0) != Y.shape[1]:
            Y = Y.as_strided(Y.shape, (Y.shape[1], 1), Y.storage_offset())
        else:
            X = X.as_strided(X.shape, (X.shape[1], 1), X.storage_offset())
    elif name == "swap_xy":           # first half-step: the X and Y fragments of 32-column block 0 in each other's registers
        def step(s, i, h, xs, ys, c):
            if s == 0 and i == 0 and h == 0:
                w = min(32, xs.shape[1], ys.shape[1])
                x2, y2 = xs.clone(), ys.clone()
                x2[:, :w], y2[:, :w] = ys[:, :w], xs[:, :w]
                c = x2.T @ y2
            return c
    else:
        raise KeyError(name)
    return _accumulate(X, Y, K, tiles, k_tile, fetch, step)


def is_noop(name, Mo, No, K, S, lay, k_tile):
    """where the wrong turn of `mutate` takes no turn at all, stated from the mutation's own definition"""
    nkt = -(-K // k_tile)
    return {"drop_row": False, "drop_last_tile": False, "swap_xy": False,
            "row_K": K % k_tile == 0,                          # no staged tile reaches row K: no zero row is read
            "tile_twice": S <= 1 or nkt == 1,                  # no second split, or none with a tile
            "stale_stage": -(-nkt // max(S, 1)) < 5,           # split 0 never re-uses a ring stage
            "swizzle": No < 16,                                # Y's row is one chunk
            "ld_as_width": K == 1 or lay == "tight",           # row 0 does not move; ld IS the width
            }[name]
