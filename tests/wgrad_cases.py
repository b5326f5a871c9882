"""Shared by test_wgrad_cases_host.py and test_gpu_wgrad_slabs.py: the 3x3 weight-gradient cases (one table over every
kernel family that writes per-split slabs for aide_wgrad_reduce_launch), their float64 reference and NaN-filled guarded
buffers.  Everything here is plain torch on the CPU; no library call.

CASES              the table: Case(family, n, ci, co, h, w, target_wgs, co_blocks, store, misaligned)
  family           'direct'    aide_conv3x3_wgrad, general kernel (four tile variants x ragged / dense)
                   'stem'      aide_conv3x3_wgrad on a stem shape (Ci <= 3, H % 4 == 0, W % 64 == 0): the folded-tap kernel
                   'stem_bf16' the same kernel through aide_conv3x3_wgrad_bf16_mixed (operands rounded to bf16 when staged)
                   'wino2'     aide_conv3x3_wgrad_wino, transposed F(2x2)
                   'wino4'     aide_conv3x3_wgrad_wino4_t, transposed F(4x4); target_wgs (0 = the library's default)
                   'bf16'      aide_conv3x3_wgrad_bf16_mixed; co_blocks 1 / 2 / 4 = the 32 / 64 / 128 co tile (0 = its rule)
  store            storage of (dz, a): 'fp32', 'bf16' (both bf16-stored) or 'dz_bf16' (bf16 dz, fp32 a): bf16 entry only
  misaligned       the case is also run with a dw that is NOT 16-byte aligned (the scalar reduce)
  Which branch of the slab reduce each shape lands on (split count, split groups, partial last workgroup) follows from the
  library's own split rules; test_wgrad_cases_host.py asks the library and fails when a required branch loses its case.
operands(case)     -> (x [N, Ci, H, W], dz [N, Co, H, W]) fp32 randn from a seeded CPU generator (values already rounded to
                   bf16 where the case stores them as bf16)
reference(case)    -> float64 dW [Co, Ci, 3, 3]: reference_dw on the operands, rounded to bf16 first for the bf16 contract
                   (DESIGN/HISTORY §4.5: bf16 operands, round to nearest even, fp32 accumulation)
guarded / guards_intact / all_pattern: a flat fp32 buffer filled with one NaN bit pattern around and inside the view"""
import collections
import functools
import zlib

import torch

Case = collections.namedtuple('Case', 'family n ci co h w target_wgs co_blocks store misaligned')

FAMILIES = ('direct', 'stem', 'stem_bf16', 'wino2', 'wino4', 'bf16')
# maximum absolute error over the maximum absolute reference value (as _close in test_gpu_kernels.py)
TOL = {'direct': 2e-5, 'stem': 2e-5, 'wino2': 2e-5, 'wino4': 1e-4, 'bf16': 3e-5, 'stem_bf16': 3e-5}


def _c(family, n, ci, co, h, w, target_wgs=0, co_blocks=0, store='fp32', misaligned=False):
    return Case(family, n, ci, co, h, w, target_wgs, co_blocks, store, misaligned)


# N * H * W stays at a few thousand pixels, with one exception per stem entry point: the stem kernel deals 4 x 64 tiles
# round-robin over min(tiles, 512) splits (at least 256), so tiles % splits != 0 needs more than 256 tiles = 65792 pixels
# (3 -> 32 channels: still microseconds on the device and milliseconds for the float64 reference).
CASES = (
    # ---- direct, variant 3 (32 co x 32 ci tile, 4-way pixel split)
    _c('direct', 1, 32, 32, 4, 16),                       # one tile: 1 split, the copy
    _c('direct', 1, 32, 32, 8, 16, misaligned=True),      # 2 splits (the smallest summing case: test_batch_boundaries)
    _c('direct', 2, 32, 32, 8, 16),                       # 4 splits, 4 groups, exactly 4 workgroups
    _c('direct', 3, 24, 36, 20, 20),                      # ragged; 30 splits, 16 groups, 864 pairs = 13.5 workgroups
    _c('direct', 1, 8, 4, 4, 16),                         # 1 split, 32 pairs < R = 1024
    _c('direct', 2, 8, 4, 8, 16),                         # 4 splits, 4 groups, 32 pairs < R = 256
    _c('direct', 1, 20, 24, 8, 32),                       # 4 splits, 4 groups, 480 pairs: 224 in the last workgroup
    _c('direct', 2, 3, 2, 32, 32, misaligned=True),       # 6 pairs: Co * Ci % 4 != 0 (scalar reduce), not a stem shape
    _c('direct', 2, 5, 7, 6, 20),                         # ragged, 35 pairs: Co * Ci % 4 != 0 with few splits
    _c('direct', 2, 32, 32, 2, 2),                        # ragged, an image smaller than one 4 x 16 tile
    # ---- direct, variant 0 (64 x 64 tile)
    _c('direct', 2, 256, 256, 12, 48),                    # 16 splits over 18 tiles: a split crosses the image boundary, 7 are empty
    _c('direct', 1, 64, 64, 6, 20),                       # ragged
    _c('direct', 2, 64, 64, 10, 10),                      # ragged, W < 16: the deepest level of a 320 x 320 input
    _c('direct', 1, 520, 130, 8, 16),                     # 2 splits, 67600 pairs: 1 group, 16 pairs in the last workgroup
    _c('direct', 2, 128, 128, 16, 64, misaligned=True),   # 32 splits, 16384 pairs (misaligned: the 64 x 16 scalar reduce)
    # ---- direct, variants 1 (32 co x 64 ci) and 2 (64 co x 32 ci), 2-way pixel split
    _c('direct', 2, 64, 32, 8, 32),
    _c('direct', 2, 72, 40, 10, 24),                      # ragged, partial tiles in both channel directions
    _c('direct', 2, 32, 64, 8, 32),
    _c('direct', 2, 40, 72, 10, 24, misaligned=True),     # ragged
    # ---- stem kernel, fp32 entry point
    _c('stem', 2, 3, 32, 64, 64, misaligned=True),        # 32 splits, 96 pairs = 64 + 32
    _c('stem', 2, 2, 20, 32, 64),                         # 16 splits, 40 pairs < R = 64; a partial co tile
    _c('stem', 1, 2, 20, 8, 128),                         # 2 x 2 tiles: 4 splits, 4 groups
    _c('stem', 3, 1, 40, 4, 64),                          # 3 tiles, 3 splits; two co tiles, the second partial
    _c('stem', 2, 3, 32, 516, 64),                        # 258 tiles over 256 splits: two splits take a second tile, in image 1
    # ---- stem kernel, bf16 entry point
    _c('stem_bf16', 2, 3, 32, 64, 64, misaligned=True),
    _c('stem_bf16', 1, 3, 64, 8, 128, store='dz_bf16'),
    _c('stem_bf16', 2, 3, 32, 516, 64, store='dz_bf16'),
    # ---- transposed F(2x2): Co, Ci >= 64, H % 2 == 0, W % 4 == 0
    _c('wino2', 2, 256, 256, 6, 48),                      # 16 splits over 18 chunks: crosses the image boundary
    _c('wino2', 1, 64, 64, 6, 20, misaligned=True),       # a partial last chunk (4 of 16 columns)
    _c('wino2', 2, 72, 136, 4, 12),                       # partial tiles in both channel directions
    _c('wino2', 1, 64, 64, 2, 4),                         # the smallest supported image: one chunk, two of its eight tiles
    # ---- transposed F(4x4): Co, Ci % 32 == 0, H % 4 == 0, W % 4 == 0, H >= 8, W >= 16
    _c('wino4', 3, 64, 96, 20, 16),                       # default target; Co % 64 == 32; 15 chunks over 7 splits (odd ranges)
    _c('wino4', 1, 32, 32, 8, 20, misaligned=True),       # Co = 32: only the half tile; a partial last chunk
    _c('wino4', 2, 64, 64, 8, 40, target_wgs=6),          # explicit target: 3 splits
    _c('wino4', 2, 32, 160, 12, 16, target_wgs=3),        # explicit target: 1 split; Co % 64 == 32
    # ---- bf16 kernel: Co % 32 == 0, W % 32 == 0, H % 4 == 0
    _c('bf16', 3, 32, 32, 20, 32, co_blocks=1),           # 15 chunks over 7 splits: crosses image boundaries
    _c('bf16', 1, 40, 32, 8, 32, misaligned=True),        # the rule picks the 32 co tile; partial ci tile
    _c('bf16', 2, 72, 64, 8, 64, co_blocks=2, store='bf16'),
    _c('bf16', 2, 64, 96, 12, 32, co_blocks=2, store='dz_bf16'),   # the second co tile half empty
    _c('bf16', 2, 64, 128, 8, 32, co_blocks=4),
    _c('bf16', 1, 96, 256, 8, 64, co_blocks=4, store='bf16'),
    _c('bf16', 2, 16, 64, 8, 32, co_blocks=1, store='bf16'),       # 64 co on the 32 co tile
    _c('bf16', 2, 32, 32, 4, 32),                         # the smallest supported image: one chunk per image, 1 split
)


BOUNDARY_CASE = _c('direct', 1, 32, 32, 8, 16, misaligned=True)      # test_batch_boundaries: microseconds per call
assert BOUNDARY_CASE in CASES


def case_id(c):
    s = '%s-%dx%d>%d@%dx%d' % (c.family, c.n, c.ci, c.co, c.h, c.w)
    if c.target_wgs:
        s += '-t%d' % c.target_wgs
    if c.co_blocks:
        s += '-b%d' % c.co_blocks
    if c.store != 'fp32':
        s += '-' + c.store
    return s


def bf16_contract(c):
    """operands are rounded to bf16 before they are multiplied"""
    return c.family in ('bf16', 'stem_bf16')


def stored_bf16(c):
    """-> (dz stored as bf16, a stored as bf16)"""
    return c.store in ('bf16', 'dz_bf16'), c.store == 'bf16'


@functools.lru_cache(maxsize=None)
def operands(c):
    """(x, dz) fp32 on the CPU, seeded by the case's name (stable under table edits)"""
    g = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    x = torch.randn(c.n, c.ci, c.h, c.w, generator=g)
    dz = torch.randn(c.n, c.co, c.h, c.w, generator=g)
    dz_b, a_b = stored_bf16(c)
    if dz_b:
        dz = dz.bfloat16().float()
    if a_b:
        x = x.bfloat16().float()
    return x, dz


def reference_dw(x, dz):
    """float64 dW[co][ci][kh][kw] = sum_{n,h,w} dz[n][co][h][w] * x[n][ci][h+kh-1][w+kw-1]"""
    co, ci = dz.shape[1], x.shape[1]
    return torch.nn.grad.conv2d_weight(x.double(), (co, ci, 3, 3), dz.double(), padding=1)


def contract_operands(c, x, dz):
    """what the family's contract multiplies: the fp32 values, or their bf16 roundings (DESIGN/HISTORY §4.5)"""
    if bf16_contract(c):
        return x.bfloat16().double(), dz.bfloat16().double()
    return x.double(), dz.double()


@functools.lru_cache(maxsize=None)
def reference(c):
    x, dz = operands(c)
    return reference_dw(*contract_operands(c, x, dz))


def rel_err(got, ref):
    """max |got - ref| / max |ref| in float64"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-30)


# ------------------------------------------------------------------------------------------------ guarded buffers
NAN_BITS = 0x7FC5A5A5          # a quiet NaN with a payload no arithmetic produces
TAIL = 4096                    # guard words behind the view
LEAD, LEAD_MISALIGNED = 4096, 4097


def guarded(numel, lead, device):
    """-> (buf, view): a flat fp32 buffer of lead + numel + 4096 elements, every word NAN_BITS, and its inner view
    buf[lead : lead + numel].  lead = 4096 keeps the view 16-byte aligned, 4097 misaligns it on purpose."""
    buf = torch.full((lead + numel + TAIL,), NAN_BITS, dtype=torch.int32, device=device).view(torch.float32)
    return buf, buf[lead:lead + numel]


def guards_intact(buf, lead, numel):
    """the guard words on both sides of the view still hold the pattern, bit for bit"""
    w = buf.view(torch.int32)
    return bool((w[:lead] == NAN_BITS).all()) and bool((w[lead + numel:] == NAN_BITS).all())


def all_pattern(t):
    """every word of the fp32 tensor still holds the pattern"""
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())
