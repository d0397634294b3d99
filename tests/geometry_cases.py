"""Image sizes of the geometry sweep (test_geometry_cpu.py keeps the list honest on the host, test_geometry_gpu.py
runs it on the device), the kernel paths they must take, and Python mirrors of the straddle predicates.

The production fp32 path is a chain of four fused kernels that hand partial maxima to each other through side
buffers; which partials go where depends on the tile grids of the image. 227x227 is one point of that space."""
from anx.config import blocks_dims
from anx.parallel.plan import full_plan

# AlexNetBlocks.last_path() of ...
# ... the whole chain fused: pool1 in the one-kernel Conv1's epilogue, pool2 in the F(4x4,5x5) GEMM's epilogue
FULL = {"conv1": "fused_pool", "pool1": "conv1_epilogue", "conv2": "f45", "pool2": "gemm_epilogue"}
# ... the one-kernel Conv1 writing its map, pool1 in the Conv2 input transform, pool2 + LRN in a kernel of their own
MIDDLE = {"conv1": "fused", "pool1": "input_transform", "conv2": "f45", "pool2": "kernel"}
# ... stage1 + stage2: pool1 and pool2 as kernels, the conv2 window materialised
UNFUSED = {"conv1": "fused", "pool1": "kernel", "conv2": "f45", "pool2": "kernel"}

# (H, W): (H1, W1), (Hp1, Wp1), (Hp2, Wp2), Conv1 3x3 tiles (ty, tx), Conv2 4x4 tiles (ty, tx)
FUSED_SIZES = {
    (35, 35): ((7, 7), (3, 3), (1, 1), (3, 3), (1, 1)),        # smallest legal image; 32 images per Conv2 workgroup
    (39, 47): ((8, 10), (3, 4), (1, 1), (3, 4), (1, 1)),       # even H1 / W1; Wp1 mod 4 = 0
    (43, 59): ((9, 13), (4, 6), (1, 2), (3, 5), (1, 2)),       # one Conv2 tile row
    (51, 83): ((11, 19), (5, 9), (2, 4), (4, 7), (2, 3)),      # Wp1 mod 4 = 1
    (67, 55): ((15, 12), (7, 5), (3, 2), (5, 4), (2, 2)),      # W1 mod 3 = 0, even W1
    (63, 75): ((14, 17), (6, 8), (2, 3), (5, 6), (2, 2)),      # Hp1 mod 4 = 2 (no other size has it), even H1
    (75, 131): ((17, 31), (8, 15), (3, 7), (6, 11), (2, 4)),   # Hp1 mod 4 = 0
    (99, 63): ((23, 14), (11, 6), (5, 2), (8, 5), (3, 2)),     # tall and narrow
    (115, 147): ((27, 35), (13, 17), (6, 8), (9, 12), (4, 5)),  # even pooled output
    (131, 179): ((31, 43), (15, 21), (7, 10), (11, 15), (4, 6)),
    (163, 99): ((39, 23), (19, 11), (9, 5), (13, 8), (5, 3)),
    (195, 211): ((47, 51), (23, 25), (11, 12), (16, 17), (6, 7)),  # non-square, every map odd
    (227, 231): ((55, 56), (27, 27), (13, 13), (19, 19), (7, 7)),  # even W1 at the production grid
    (231, 227): ((56, 55), (27, 27), (13, 13), (19, 19), (7, 7)),  # even H1 at the production grid
    (271, 195): ((66, 47), (32, 23), (15, 11), (22, 16), (8, 6)),  # Hp1 = 32: the last value the 5-bit pixel decode holds
    (267, 234): ((65, 56), (32, 27), (15, 13), (22, 19), (8, 7)),  # every limit at once (Hp1 = 32, tx = 19, wq = 31)
}
# the first size past each limit of the fused chain, and the path it takes instead
FALLBACK_SIZES = {
    (227, 235): UNFUSED,  # Wp1 = 28: the padded Conv2 window is 32 columns, one more than the band transforms hold
    (227, 239): UNFUSED,  # 20 Conv1 tile columns (and a 32-column window with them: the window limit comes first)
    (275, 227): MIDDLE,   # Hp1 = 33: past the Conv1 epilogue's 5-bit pixel decode; the window still fits
    (195, 259): UNFUSED,  # 21 tile columns, a 35-column window
}
ALL_SIZES = [*FUSED_SIZES, *FALLBACK_SIZES]
# sizes also run at 40 images: workgroup boundaries (32 tiles) at many positions inside and between images
SMALL_SIZES = [hw for hw in FUSED_SIZES if hw[0] <= 99 and hw[1] <= 131]  # up to 99 x 63 in the table's order
N_SWEEP, N_SMALL = 9, 40  # 9: the smallest batch above the Auto crossover (Winograd above 8 images per launch)

CONV1_WG_TILES = 32  # anx::hip::kConv1FusedTiles
CONV2_WG_TILES = 32  # anx::hip::kConv2PoolTiles


# The two predicates below follow csrc/include/anx/ops.hpp:154-189 (pool1_straddles / pool2_straddles) line by line.
def pool1_straddles(n: int, py: int, px: int, ty1: int, tx1: int) -> bool:
    b = n * ty1 * tx1
    gm = b + (2 * py // 3) * tx1 + (2 * px) // 3
    gM = b + ((2 * py + 2) // 3) * tx1 + (2 * px + 2) // 3
    return gm // CONV1_WG_TILES != gM // CONV1_WG_TILES


def pool2_straddles(n: int, py: int, px: int, ty2: int, tx2: int) -> bool:
    gm = n * ty2 * tx2 + (py >> 1) * tx2 + (px >> 1)
    gM = gm + (tx2 if py & 1 else 0) + (px & 1)
    return gm // CONV2_WG_TILES != gM // CONV2_WG_TILES


def launch_grids(H: int, W: int):
    """The tile grids the whole-image forward launches with: ((ty1, tx1), (ty2, tx2)). The whole-image tile holds
    the rows its output needs (a pool drops the last row of an even map), so the row counts come from the plan."""
    d, t = blocks_dims(H, W), full_plan(H, W)
    return ((-(-t.c1.size // 3), -(-d.W1 // 3)), (-(-t.c2.size // 4), -(-d.W2 // 4)))


def straddle_counts(H: int, W: int, N: int):
    """(straddling pool1 windows, pool1 pixels, straddling pool2 windows, pool2 pixels) of an N-image launch."""
    d, t = blocks_dims(H, W), full_plan(H, W)
    (ty1, tx1), (ty2, tx2) = launch_grids(H, W)
    s1 = sum(pool1_straddles(n, py, px, ty1, tx1) for n in range(N) for py in range(t.p1.size) for px in range(d.Wp1))
    s2 = sum(pool2_straddles(n, py, px, ty2, tx2) for n in range(N) for py in range(d.Hp2) for px in range(d.Wp2))
    return s1, N * t.p1.size * d.Wp1, s2, N * d.Hp2 * d.Wp2
