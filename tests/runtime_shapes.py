"""Shape tables of tests/test_runtime_shapes_gpu.py, built from the tile constants of the kernels that take their sizes at run time
(csrc/plin.hip, glinear.hip, gconv.hip, c1d.hip), and plain-Python mirrors of the host-side routing those tables are aimed at.  No
torch, no GPU: the tables can be inspected (and their own claims checked) anywhere."""

# ---- tile constants, as the kernels name them -------------------------------------------------------------------------------------------
PLIN_TILE = 128        # plin.hip / glinear.hip: 128 rows x 128 columns per workgroup
PLIN_KBLOCK = 32       # k-blocks of 32, k-groups of 16
PLIN_MIN_K, PLIN_MIN_N, PLIN_MIN_ROWS = 128, 64, 128   # linear_uses_planes
GCONV_ROWS, GCONV_COLS, GCONV_KBLK = 64, 256, 16       # gconv.hip: 64 rows x 256 columns, KBLK = 16
THIN_MAX_TAPS, THIN_COUT, THIN_WGS = 6, 32, 512        # thin_wgrad_kernel
C1D_CHUNK = 64         # c1d.hip: positions per wave of its weight gradient
POOL_QUADS, POOL_THREADS = 4, 256                      # the max-pool backward kernels: 4 quads (or pairs) per thread


def round_up(x, m):
    return (x + m - 1) // m * m


def uses_planes(n, K, N):
    return K >= PLIN_MIN_K and N >= PLIN_MIN_N and n >= PLIN_MIN_ROWS


# ---- A1: the dense boundary grid ----------------------------------------------------------------------------------------------------
DENSE_ROWS = [
    1,      # one row: a single clamped row in a 128-row tile
    127,    # one short of the plane family's 128 rows: the largest f32 launch of a plane layer
    128,    # the smallest plane launch, exactly one row tile
    129,    # one row into the second row tile
    257,    # one row into the third row tile
]
DENSE_K = [
    128,    # smallest plane K: four whole k-blocks
    129,    # one column into a k-block, not a multiple of 4 (ld_in rounds up to 132)
    131,    # last column of a 4-float load inside the first k-group
    132,    # a multiple of 4 that is no multiple of the k-group
    159,    # one short of a whole k-block, inside the second k-group
    160,    # exactly five k-blocks
    161,    # one column past a k-block boundary
    257,    # one column past two column tiles of the data gradient
]
DENSE_N = [
    64,     # smallest plane N: half a column tile, two k-blocks of the data gradient
    68,     # one 4-float load past 64: the data gradient's last k-block holds 4 of 32
    124,    # one load short of a column tile
    128,    # exactly one column tile
    132,    # one load into the second column tile
    260,    # one load past two column tiles
]
# leading-dimension slack, cycled over the grid: none, one load, more than a k-block
DENSE_SLACK = [0, 4, 40]


def dense_grid():
    """Pairwise cover of DENSE_ROWS x DENSE_K x DENSE_N: every (K, N) pair once, rows rotated so that every (n, K) and every (n, N)
    pair occurs too; plus the two smallest f32 layers.  Entries: (n, K, N, ld_in, ld_dout, ld_out)."""
    cases = []
    for i, K in enumerate(DENSE_K):
        for j, N in enumerate(DENSE_N):
            n = DENSE_ROWS[(i + j) % len(DENSE_ROWS)]
            t = i * len(DENSE_N) + j
            ld_in = round_up(K, 4) + DENSE_SLACK[t % 3]
            ld_dout = N + DENSE_SLACK[(t + i + 1) % 3]
            ld_out = N + (1, 7, 0)[t % 3] + 4        # output rows need no alignment: an odd stride is legal
            cases.append((n, K, N, ld_in, ld_dout, ld_out))
    cases.append((1, 1, 4, 8, 8, 5))      # the smallest f32 layer: one row, one input column, one 4-float output load
    cases.append((3, 5, 8, 12, 8, 11))    # K and n below every tile constant, K not a multiple of 4
    return cases


def _pairs(cases, a, b):
    return {(c[a], c[b]) for c in cases}


def dense_grid_is_pairwise(cases):
    grid = [c for c in cases if c[1] >= PLIN_MIN_K]
    return (len(_pairs(grid, 0, 1)) == len(DENSE_ROWS) * len(DENSE_K) and len(_pairs(grid, 0, 2)) == len(DENSE_ROWS) * len(DENSE_N)
            and len(_pairs(grid, 1, 2)) == len(DENSE_K) * len(DENSE_N))


def amax_ranges(K):
    """Column ranges [lo, hi) of din_amax (lo a multiple of 4): inside one 128-column tile, ending at K, and -- where K is no multiple
    of 4 -- starting in the last 4-float group so that the range ends at K inside a load."""
    out = [(4, min(K, 100))] if K > 4 else []
    out.append(((K // 2) // 4 * 4, K))
    out.append(((K - 1) // 4 * 4, K))
    return [r for r in dict.fromkeys(out) if r[0] < r[1]]


# ---- B: convolutions -----------------------------------------------------------------------------------------------------------------
def conv_out(h, w, kh, kw, s, pad):
    return (h + 2 * pad[0] - kh) // s + 1, (w + 2 * pad[1] - kw) // s + 1


def conv_is_c1d(shape):
    n, cin, h, w, cout, kh, kw, s, pad = shape
    return h == 1 and kh == 1 and s == 2 and pad == (0, 0) and cout == 32 and (cin, kw) in ((1, 5), (32, 3))


def conv_is_first(shape):
    n, cin, h, w, cout, kh, kw, s, pad = shape
    return s == 1 and h == 48 and w == 48 and kh == kw and pad == (1, 1) and cout == 64 and (kh, cin) in ((7, 3), (3, 1), (3, 4))


def conv_is_planes(shape):
    n, cin, h, w, cout, kh, kw, s, pad = shape
    if s != 1 or h != w or kh != kw or pad[0] != pad[1]:
        return False
    layer = (cin, cout, kh, h)
    if pad[0] == 0:
        return layer == (64, 64, 3, 9)
    return pad[0] == 1 and layer in ((64, 128, 5, 22), (128, 256, 3, 10), (64, 128, 3, 24), (128, 256, 3, 12))


def conv_is_specialised(shape):
    return conv_is_c1d(shape) or conv_is_first(shape) or conv_is_planes(shape)


def conv_is_thin(shape):
    n, cin, h, w, cout, kh, kw, s, pad = shape
    oh, _ = conv_out(h, w, kh, kw, s, pad)
    return kh == 1 and h == 1 and oh == 1 and cin * kw <= THIN_MAX_TAPS and cout <= THIN_COUT and pad[0] == 0


def conv_wgrad_split_ranges(shape):
    """[begin, end) in k-blocks of every split of the gather weight gradient (conv_wgrad_splits + Wgrad::init of csrc/gconv.hip)."""
    n, cin, h, w, cout, kh, kw, s, pad = shape
    oh, ow = conv_out(h, w, kh, kw, s, pad)
    KT = cin * kh * kw
    tiles = ((KT + 255) // 256) * ((cout + 63) // 64)
    S = (768 + tiles - 1) // tiles
    nkb = (n * oh * ow + GCONV_KBLK - 1) // GCONV_KBLK
    S = max(1, min(S, (nkb + 7) // 8))
    per = (nkb + S - 1) // S
    return [(min(nkb, i * per), min(nkb, min(nkb, i * per) + per)) for i in range(S)]


# (n, cin, h, w, cout, kh, kw, stride, (pad_h, pad_w)) -- each entry sits on one boundary of the 64 x 256 x 16 gather tiles
CONV_GEOMETRIES = [
    (2, 3, 9, 9, 1, 3, 3, 1, (1, 1)),      # cout = 1: one live row in a 64-row tile
    (2, 3, 9, 9, 63, 3, 3, 1, (1, 1)),     # cout = 63: one short of a row tile
    (2, 3, 8, 8, 64, 3, 3, 1, (1, 1)),     # cout = 64: exactly one row tile (8 x 8: not a plane geometry)
    (2, 3, 9, 9, 65, 3, 3, 1, (1, 1)),     # cout = 65: one row into the second row tile
    (3, 5, 7, 9, 6, 1, 3, 1, (0, 1)),      # cin kh kw = 15: one short of a k-block of 16; 1 x k kernel, padding on the w axis only
    (3, 4, 8, 8, 6, 2, 2, 1, (0, 0)),      # cin kh kw = 16: exactly one k-block
    (3, 17, 7, 7, 6, 1, 1, 1, (0, 0)),     # cin kh kw = 17: one tap into the second k-block; 1 x 1 kernel
    (3, 11, 8, 7, 6, 3, 1, 1, (1, 0)),     # cin kh kw = 33: one tap into the third k-block; k x 1 kernel, padding on the h axis only
    (5, 2, 5, 19, 7, 3, 3, 1, (0, 0)),     # n oh ow = 5 x 3 x 17 = 255: one short of a column tile
    (4, 2, 10, 10, 7, 3, 3, 1, (0, 0)),    # n oh ow = 256: exactly one column tile (8 x 8 per sample)
    (1, 2, 259, 3, 7, 3, 3, 1, (0, 0)),    # n oh ow = 257: one column into the second column tile
    (3, 3, 13, 13, 8, 3, 3, 2, (1, 1)),    # stride 2, padding 1
    (3, 3, 13, 14, 8, 5, 5, 2, (2, 2)),    # stride 2, padding 2, w + 2p - k odd: the last input column is never read
    (3, 3, 29, 29, 8, 4, 4, 4, (1, 1)),    # stride 4, padding 1: (29 + 2 - 4) % 4 = 3 unread rows and columns
    (3, 3, 22, 23, 8, 5, 5, 4, (2, 2)),    # stride 4, padding 2: 1 unread row, 2 unread columns
    (2, 2, 16, 11, 5, 3, 2, 2, (0, 0)),    # stride 2 without padding: one unread row ((16 - 3) % 2) and column ((11 - 2) % 2), kh != kw
    (2, 2, 6, 7, 5, 2, 2, 1, (2, 3)),      # padding >= the kernel size: the outermost outputs see padding only and equal the bias
    (3, 2, 1, 40, 5, 1, 4, 1, (0, 4)),     # the same on a single-row input (Conv1d), padding = kw: not thin (cin kw = 8)
    (3, 2, 6, 10, 9, 3, 3, 1, (0, 0)),     # oh ow = 32: the smallest plane the weight gradient takes; k-blocks align with samples
    (3, 2, 5, 13, 9, 3, 3, 1, (0, 0)),     # oh ow = 33: every k-block after the first straddles two samples
    (3, 2, 7, 9, 9, 3, 3, 1, (0, 0)),      # oh ow = 35
    (3, 2, 3, 49, 9, 3, 3, 1, (0, 0)),     # oh ow = 47: one short of three k-blocks
    (4, 2, 6, 9, 4, 2, 2, 1, (0, 0)),      # n oh ow = 160 = 10 k-blocks in 2 splits of 5: the even case next to the two below
    (5, 2, 7, 9, 4, 3, 3, 1, (0, 0)),      # 175 outputs = 11 k-blocks in 2 splits of 6 and 5, the last block holds 15 of 16: uneven last split
    (2810, 1, 8, 10, 4, 4, 4, 1, (0, 0)),  # 98,350 outputs = 6,147 k-blocks over 768 splits of 9: the last 85 splits are empty
    (2, 70, 6, 6, 66, 2, 2, 1, (1, 1)),    # cin = 70, cout = 66: two row tiles in the forward, the data and the weight gradient
    (2, 29, 7, 7, 3, 3, 3, 1, (1, 1)),     # cin kh kw = 261: the weight gradient's taps cross its 256-column tile
]
# the c1d item: Conv1d(32, 32, 3, stride 2) of csrc/c1d.hip at run-time widths, output lengths around its 64-position chunk
C1D_WIDTHS = [
    (3, 127),    # ow = 63: one short of a chunk
    (3, 130),    # ow = 64: exactly one chunk, even width: the last input column is never read
    (3, 131),    # ow = 65: one position into the second chunk
    (2, 259),    # ow = 129: one position into the third chunk
]


def c1d_shape(n, w):
    return (n, 32, 1, w, 32, 1, 3, 2, (0, 0))


# B2: three of the geometries above in strided sample records; (index into CONV_GEOMETRIES, extra floats per input / output sample)
CONV_STRIDED = [
    (3, 2, 2),     # cout = 65: sample strides 243 + 2 and 5265 + 2
    (13, 7, 5),    # stride 4 with unread rows and columns: 2523 + 7 and 392 + 5
    (19, 1, 9),    # oh ow = 33, straddling k-blocks of the weight gradient: 130 + 1 and 297 + 9
]
# B3: oh ow < 32 -- the weight gradient is unsupported; forward and data gradient work
CONV_SMALL_PLANES = [
    (3, 4, 7, 7, 6, 3, 3, 1, (0, 0)),     # oh ow = 25
    (2, 3, 12, 12, 5, 2, 2, 2, (0, 0)),   # oh ow = 36 -> the control: supported (next to 31 below)
    (2, 3, 1, 33, 5, 1, 3, 1, (0, 0)),    # oh ow = 31: one short
]

# B4: thin weight gradient (h = kh = 1, cin kw <= 6, cout <= 32): (n, cin, w, cout, kw, stride, pad_w)
THIN = [
    (7, 1, 40, 5, 1, 1, 0),      # KT = 1
    (7, 1, 64, 32, 2, 2, 0),     # KT = 2, cout = 32, ow = 32: the smallest plane
    (1, 2, 129, 1, 1, 4, 2),     # KT = 2 as cin = 2, kw = 1; cout = 1, stride 4, padded (stride 4 needs w > 124 for ow >= 32)
    (7, 1, 70, 5, 3, 2, 2),      # KT = 3, padded
    (1, 3, 45, 32, 1, 1, 0),     # KT = 3 as three channels of one tap
    (7, 2, 67, 1, 2, 2, 0),      # KT = 4, cout = 1
    (1, 1, 66, 32, 4, 1, 2),     # KT = 4 as one channel
    (7, 1, 69, 5, 5, 2, 2),      # KT = 5 (cout = 5: not the c1d first layer)
    (515, 1, 43, 32, 5, 1, 0),   # KT = 5, more samples than THIN_WGS = 512 workgroups: the b += gridDim.x loop runs twice for 3 of them
    (7, 2, 70, 32, 3, 2, 0),     # KT = 6 as cin = 2, kw = 3
    (7, 3, 68, 5, 2, 1, 2),      # KT = 6 as cin = 3, kw = 2
    (515, 3, 40, 1, 2, 1, 0),    # KT = 6, n > THIN_WGS, cout = 1
    (1, 2, 133, 5, 3, 4, 2),     # KT = 6, stride 4, padded, one sample, two unread columns
]
# just outside: the same kind of layer on the MFMA weight gradient
NOT_THIN = [
    (7, 7, 50, 32, 1, 1, 0),     # KT = 7
    (7, 2, 70, 33, 3, 2, 0),     # cout = 33
]


def thin_shape(t):
    n, cin, w, cout, kw, s, pw = t
    return (n, cin, 1, w, cout, 1, kw, s, (0, pw))


# ---- C: max-pool ---------------------------------------------------------------------------------------------------------------------
# ((n, c), h, w); quads = n c h w / 4 (4 per thread, 1,024 per workgroup of the quad kernel), pairs = quads / 2 (the W % 4 == 0 kernel)
POOLS = [
    ((1, 3), 22, 22),     # W % 4 == 2: 363 quads, one partial workgroup
    ((1, 7), 26, 30),     # W % 4 == 2: 1,365 quads = one whole workgroup + 341
    ((1, 5), 20, 24),     # W % 4 == 0: 300 pairs, one partial workgroup
    ((11, 1), 20, 44),    # W % 4 == 0: 1,210 pairs = one whole workgroup + 186
    ((2, 2), 2, 4),       # W % 4 == 0, one row pair per plane: 2 pairs in all
    ((1, 1), 2, 2),       # a single window
    ((1, 2), 4, 6),       # W % 4 == 2 and a quad that spans two rows
]
