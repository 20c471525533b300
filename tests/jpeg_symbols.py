"""Designed frames for the JPEG entropy coder (csrc/jpeg.hip: lane_bits, jpeg_code_kernel's count and emit forms and the stuffing kernels), and
a report of what a set of frames makes the coder emit.  NumPy only; everything is deterministic from this code, nothing is read from a file.

Random content reaches about two thirds of the luma and two fifths of the chroma run/size symbols, no chroma DC category 11 and lane
patterns of 50 bits.  The frames here are mosaics of blocks built for one symbol each: the inverse DCT of a chosen quantised coefficient
(or two) times its quantisation step, rounded and clipped to uint8.  Rounding and clipping add coefficients of their own, so a block is
KEPT only if the restatement's ``scan_blocks`` (tests/jpeg_ref.py), run on the pixels, gives the run/size symbol that was aimed at, at the
position aimed at - never on the strength of the target alone.  ``coverage`` then counts, from ``scan_blocks`` and ``entropy_bits``
alone, what the frames reach; tests/test_jpeg_symbols_host.py asserts the counts and tests/test_gpu_jpeg_symbols.py holds the device to
the restatement and to Pillow on these frames.
"""
import functools

import numpy as np

import jpeg_ref as J

QUALITIES = (75, 90, 95, 98, 100)          # a target is tried at each, in this order, and kept at the first that codes it
SIDE = 320                                 # the mosaics are SIDE x SIDE: 1600 blocks (L) or 400 MCUs (RGB)
CHUNK = 1024                               # bytes of unstuffed stream per pass of the stuffing kernels (CHUNK in csrc/jpeg.hip)
LUMA, CHROMA = 0, 1
SIZES = range(1, 11)

_k = np.arange(8)
_C = np.sqrt(np.where(_k == 0, 1, 2) / 8.0)[:, None] * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16)      # orthonormal DCT-II [u, x]


def target_samples(targets, table, quality):
    """The float samples (level shift undone) whose DCT has value * step at each (zigzag position, quantised value) and 0 elsewhere.
    libjpeg's coefficients are the orthonormal DCT's scaled by 8 and its divisor is 8 q, so the orthonormal coefficient is value * q."""
    q = J.quant_table(J.Q_CHROMA if table == CHROMA else J.Q_LUMA, quality)
    coef = np.zeros(64)
    for p, v in targets:
        coef[J.ZIGZAG[p]] = v * q[J.ZIGZAG[p]]
    return _C.T @ coef.reshape(8, 8) @ _C + 128.0


def _u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def grey_block(targets, quality):
    """uint8 [8, 8]."""
    return _u8(target_samples(targets, LUMA, quality))


def chroma_block(targets, quality, line=False, shift=0.0):
    """uint8 [16, 16, 3]: the Cb samples replicated 2 x 2.  ``line`` False: Y = Cr = 128 (R = 128, G = 128 - 0.34414 d, B = 128 + 1.772 d for
    d = Cb - 128; in gamut for |d| <= 71).  ``line`` True: the colours between yellow (255, 255, 0), Cb 0, and blue (0, 0, 255), Cb 255,
    on which Cb = 0.5 + 255 t: the whole range of Cb, with Y and Cr moving along."""
    cb = np.repeat(np.repeat(target_samples(targets, CHROMA, quality), 2, axis=0), 2, axis=1) + shift
    if line:
        t = np.clip((cb - 0.5) / 255.0, 0, 1)
        return _u8(np.stack([255 * (1 - t), 255 * (1 - t), 255 * t], axis=-1))
    d = cb - 128.0
    return _u8(np.stack([np.full_like(d, 128.0), 128 - 0.344136 * d, 128 + 1.772 * d], axis=-1))


def _value(size, sign):
    """A quantised value of that size, 1.25 * 2^(size - 1) rounded: a quarter of the way into the size's range, so that rounding and
    clipping leave the size alone."""
    return sign * max(1, int(1.25 * (1 << (size - 1))))


def _targets():
    """(kind, run, size, sign, targets): one coefficient behind the DC at every position (run 0..62: position 63 alone is the last of
    them), and the same run/size behind a small coefficient at position 1 or 3 instead of behind the DC."""
    out = []
    for size in SIZES:
        for sign in (1, -1):
            for run in range(63):
                out.append(("one", run, size, sign, [(run + 1, _value(size, sign))]))
            for first in (1, 3):
                for run in range(63 - first):
                    out.append((f"two{first}", run, size, sign, [(first, -sign), (first + run + 1, _value(size, sign))]))
    return out


def _mosaic(blocks, per_row):
    """Blocks [k, s, s(, 3)] -> one image with per_row of them a row, the last row filled with mid grey."""
    k, s = len(blocks), blocks.shape[1]
    rows = -(-k // per_row)
    full = np.full((rows * per_row,) + blocks.shape[1:], 128, np.uint8)
    full[:k] = blocks
    full = full.reshape((rows, per_row) + blocks.shape[1:])
    return np.ascontiguousarray(full.swapaxes(1, 2).reshape((rows * s, per_row * s) + blocks.shape[3:]))


def _coded(pixels, table, quality):
    """For candidate blocks [k, 8, 8] / [k, 16, 16, 3]: (coded, run, size) [k, 64] of the luma block / the Cb block as scan_blocks sees it."""
    z, tbl = J.scan_blocks(_mosaic(pixels, 64), quality)
    if table == CHROMA:
        z = z.reshape(-1, 6, 64)[:, 4]
    nz, run, size, _ = J.run_sizes(z[:len(pixels)].copy())
    return nz, run, size, z[:len(pixels)]


@functools.lru_cache(maxsize=None)
def designed_blocks(table):
    """The kept blocks of a table as a list of (quality, kind, run, size, sign, pixels): every target of ``_targets`` at the first
    quality of QUALITIES (chroma: Y = Cr = 128 first, then the yellow-blue line) at which scan_blocks codes (run & 15, size) with that
    run at the target's position and nothing but the target's coefficients in front of it."""
    todo = _targets()
    kept = []
    for quality in QUALITIES:
        for line in ((False, True) if table == CHROMA else (False,)):
            if not todo:
                break
            if table == CHROMA:
                pixels = np.stack([chroma_block(t[4], quality, line) for t in todo])
            else:
                pixels = np.stack([grey_block(t[4], quality) for t in todo])
            nz, run, size, z = _coded(pixels, table, quality)
            left = []
            for i, t in enumerate(todo):
                kind, r, s, sign, targets = t
                p = targets[-1][0]
                ok = nz[i, p] and run[i, p] == r and size[i, p] == s and np.sign(z[i, p]) == sign
                ok = ok and all(nz[i, pp] for pp, _ in targets) and int(nz[i, 1:p].sum()) == len(targets) - 1
                if ok:
                    kept.append((quality, kind, r, s, sign, pixels[i]))
                else:
                    left.append(t)
            todo = left
    return kept + _sweep(table, todo, kept)


SWEEP_VALUES = 32                                     # values tried per target of the sweep, spread over the size's range
SWEEP_SHIFTS = (0.0, 0.25, -0.25, 0.5)                # and, per value, these offsets of every sample before rounding


def _sweep(table, todo, kept):
    """The second search, at quality 100 (every step is 1) for the one-coefficient targets the first left over that matter most: those
    behind three ZRLs (run >= 48), and those whose (run & 15, size) nothing kept so far codes.  At a step of 1 the rounding of the
    samples alone (an error of about 0.3 per coefficient) codes some of the 48 and more coefficients that must stay zero, so one
    value per size is not enough: SWEEP_VALUES values of the size, up to 530 (beyond it the samples clip), each at SWEEP_SHIFTS
    offsets that change how the samples round.  Behind three ZRLs a block is kept only if the target is its only AC coefficient, so
    that the EOB lands in the same lane pattern.  First hit per target, in a fixed order."""
    quality = 100
    reached = {(r & 15, s) for _, _, r, s, _, _ in kept}
    todo = [t for t in todo if t[0] == "one" and (t[1] >= 48 or (t[1] & 15, t[2]) not in reached)]
    found = []
    for k in range(SWEEP_VALUES):
        if not todo:
            break
        value = lambda s, k: (1 << (s - 1)) + (min((1 << s) - 1, 530) - (1 << (s - 1))) * k // (SWEEP_VALUES - 1)
        idle = [t for t in todo if k and value(t[2], k) == value(t[2], k - 1)]          # a small size has fewer values than rounds
        todo = [t for t in todo if not (k and value(t[2], k) == value(t[2], k - 1))]
        if not todo:
            todo = idle
            continue
        cands = []
        for t in todo:
            _, r, s, sign, _ = t
            v = sign * value(s, k)
            for shift in SWEEP_SHIFTS:
                if table == CHROMA:
                    cands.append(chroma_block([(r + 1, v)], quality, line=True, shift=shift))
                else:
                    cands.append(_u8(target_samples([(r + 1, v)], LUMA, quality) + shift))
        nz, run, size, z = _coded(np.stack(cands), table, quality)
        left = []
        for i, t in enumerate(todo):
            _, r, s, sign, _ = t
            p = r + 1
            for j in range(len(SWEEP_SHIFTS) * i, len(SWEEP_SHIFTS) * (i + 1)):
                ok = nz[j, p] and run[j, p] == r and size[j, p] == s and np.sign(z[j, p]) == sign
                if ok and (r < 48 or int(nz[j, 1:].sum()) == 1):
                    found.append((quality, "one", r, s, sign, cands[j]))
                    break
            else:
                left.append(t)
        todo = left + idle
    return found


# ---- DC ladders -------------------------------------------------------------------------------------------------------------------------
STEPS = (0, 1, 2, 3, 5, 8, 12, 20, 32, 48, 80, 128, 192, 255)


def _ladder():
    """Levels 0..255 whose neighbours differ by every step of STEPS, up and down: low, low + d, low for each d."""
    levels = []
    for d in STEPS:
        low = max(0, 128 - d // 2 - 1)
        levels += [low, min(255, low + d), low]
    return np.array(levels)


def dc_ladder(mode):
    """Constant blocks (L) or MCUs (RGB).  L: the grey levels of the ladder, then 0 and 255 alternating: at quality 100 a DC difference of
    +-2040, category 11.  RGB: the same greys (luma DC, chroma constant), then the colours (255 - c, 255 - c, c), whose Cb is c, for the
    ladder's c, then pure yellow (255, 255, 0) and pure blue (0, 0, 255) alternating: chroma DC difference +-2040."""
    lv = np.concatenate([_ladder(), np.tile([0, 255], 4)])
    if mode == "L":
        return np.broadcast_to(lv[:, None, None], (len(lv), 8, 8)).astype(np.uint8)
    grey = np.stack([lv, lv, lv], axis=-1)
    colour = np.stack([255 - lv, 255 - lv, lv], axis=-1)
    px = np.concatenate([grey, colour])
    return np.broadcast_to(px[:, None, None, :], (len(px), 16, 16, 3)).astype(np.uint8)


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(mode):
    """The designed frames of a mode ("L": [SIDE, SIDE], "RGB": [SIDE, SIDE, 3]) as a tuple of (name, quality, read-only uint8 image).  Per
    quality the kept blocks in the order of ``_targets``, cut into mosaics of one shape - the last one of a quality is part mid grey - and per quality one
    frame that starts with the DC ladder and goes on with every third of that quality's blocks from the other end, which puts the same
    blocks at other bit offsets and makes the files of one shape and quality differ in length by a lot.  Last, ``dense_frame``."""
    table = LUMA if mode == "L" else CHROMA
    s = 8 if mode == "L" else 16
    per_row = SIDE // s
    per_frame = per_row * per_row
    out = []
    for quality in QUALITIES:
        blocks = [b[5] for b in designed_blocks(table) if b[0] == quality]
        ladder = dc_ladder(mode)
        parts = [np.stack(blocks[a:a + per_frame]) for a in range(0, len(blocks), per_frame)]
        parts.append(np.concatenate([ladder, np.stack(blocks[::-1][::3][:per_frame - len(ladder)])]))
        for i, part in enumerate(parts):
            img = _mosaic(part, per_row)
            img = np.concatenate([img, np.full((SIDE - img.shape[0],) + img.shape[1:], 128, np.uint8)])
            img.setflags(write=False)
            out.append((f"{mode}-q{quality}-{i}", quality, img))
    dense = dense_frame(mode)
    dense.setflags(write=False)
    out.append((f"{mode}-q100-dense", 100, dense))
    return tuple(out)


def dense_frame(mode):
    """Random 0 / 255 samples, for quality 100: not built for a symbol but for bits.  One-coefficient blocks make short streams (100 bits
    a block at most); at a step of 1 this frame codes every coefficient of every block, 936 (L) and 776 (RGB) bits a block against the
    348 and 260 of the same content at quality 75, the densest stream of tests/test_gpu_jpeg.py, and the 1660 of max_block_bits."""
    rng = np.random.default_rng(20 if mode == "L" else 21)
    return (rng.integers(0, 2, (SIDE, SIDE) if mode == "L" else (SIDE, SIDE, 3), dtype=np.uint8) * 255).astype(np.uint8)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def unstuffed(pat, ln):
    """The bytes of the stream before stuffing, the last one padded with 1-bits: what the stuffing kernels read in chunks of CHUNK."""
    return np.frombuffer(J.pack_bits(pat, ln).replace(b"\xff\x00", b"\xff"), np.uint8)


def _empty_table():
    return {"dc": set(), "ac": set(), "chains": {}, "ends_at_63": False}


def coverage(images, quality):
    """What the entropy coder is asked to emit for these images at this quality, from scan_blocks and entropy_bits alone:
    {"luma" / "chroma": {"dc": the DC categories, "ac": the (run & 15, size) symbols, "chains": {ZRLs in front of a symbol: the sizes
    coded behind that many}, "ends_at_63": a block whose coefficient 63 is coded (no EOB)}, "longest": the longest lane pattern in bits,
    "offsets": the bit offsets pos & 31 at which a pattern longer than 32 bits starts, "ff_last" / "ff_first": some 0xFF byte of the
    unstuffed stream is the last / the first byte of a CHUNK-byte chunk, "ff_both": both in one frame}."""
    cov = {"luma": _empty_table(), "chroma": _empty_table(), "longest": 0, "offsets": set(), "ff_last": False, "ff_first": False, "ff_both": False}
    for img in images:
        z, tbl = J.scan_blocks(img, quality)
        nz, run, size, _ = J.run_sizes(z.copy())
        pat, ln = J.entropy_bits(z, tbl)
        for t, name in ((LUMA, "luma"), (CHROMA, "chroma")):
            m = tbl == t
            if not m.any():
                continue
            c = cov[name]
            c["dc"] |= set(size[m, 0].tolist())
            ac = nz[m, 1:]
            r, s = run[m, 1:][ac], size[m, 1:][ac]
            c["ac"] |= set(zip((r & 15).tolist(), s.tolist()))
            for k, sz in set(zip((r >> 4).tolist(), s.tolist())):
                c["chains"].setdefault(k, set()).add(sz)
            c["ends_at_63"] = c["ends_at_63"] or bool(nz[m, 63].any())
        flat = ln.reshape(-1)
        start = np.cumsum(flat) - flat
        cov["longest"] = max(cov["longest"], int(flat.max()))
        cov["offsets"] |= set((start[flat > 32] & 31).tolist())
        ff = np.nonzero(unstuffed(pat, ln) == 0xFF)[0] % CHUNK
        last, first = bool((ff == CHUNK - 1).any()), bool((ff == 0).any())
        cov["ff_last"], cov["ff_first"], cov["ff_both"] = cov["ff_last"] or last, cov["ff_first"] or first, cov["ff_both"] or (last and first)
    return cov


def merge(covs):
    """The union of several coverage results."""
    out = {"luma": _empty_table(), "chroma": _empty_table(), "longest": 0, "offsets": set(), "ff_last": False, "ff_first": False, "ff_both": False}
    for cov in covs:
        for name in ("luma", "chroma"):
            a, b = out[name], cov[name]
            a["dc"] |= b["dc"]
            a["ac"] |= b["ac"]
            for k, v in b["chains"].items():
                a["chains"].setdefault(k, set()).update(v)
            a["ends_at_63"] = a["ends_at_63"] or b["ends_at_63"]
        out["longest"] = max(out["longest"], cov["longest"])
        out["offsets"] |= cov["offsets"]
        for k in ("ff_last", "ff_first", "ff_both"):
            out[k] = out[k] or cov[k]
    return out


def frames_coverage(mode):
    """Of a mode's mosaics, each at its quality; the dense frame is left out: what is counted is what was built."""
    fr = [f for f in frames(mode) if not f[0].endswith("dense")]
    return merge(coverage([f[2] for f in fr if f[1] == q], q) for q in sorted({f[1] for f in fr}))


@functools.lru_cache(maxsize=None)
def designed_coverage():
    """Of all designed frames, both modes, each at its quality."""
    return merge([frames_coverage("L"), frames_coverage("RGB")])


@functools.lru_cache(maxsize=None)
def old_fixture_coverage():
    """Of the fixtures of tests/test_gpu_jpeg.py's byte tests: J.SHAPES x J.CONTENTS x {RGB, L} at quality 75 and test_other_qualities'
    6 qualities x 3 shapes x 3 kinds."""
    covs = [coverage([J.content(kind, h, w, c) for (h, w) in J.SHAPES for c in (3, 1) for kind in J.CONTENTS], 75)]
    for quality in (1, 30, 50, 90, 95, 100):
        covs.append(coverage([J.content(kind, h, w, c) for (h, w) in [(17, 9), (37, 53), (250, 333)] for c in (3, 1)
                              for kind in ("noise", "smooth", "binary")], quality))
    return merge(covs)


ALL_AC = frozenset((r, s) for r in range(16) for s in SIZES)


def report(cov, title):
    """The coverage table as text."""
    lines = [title]
    for name in ("luma", "chroma"):
        c = cov[name]
        missing = sorted(ALL_AC - c["ac"])
        lines.append(f"  {name}: DC categories {sorted(c['dc'])}; {len(c['ac'] & ALL_AC)} of 160 AC symbols; not reached: {missing}")
        lines.append(f"  {name}: sizes behind k ZRLs: " + "; ".join(f"{k}: {sorted(v)}" for k, v in sorted(c["chains"].items()))
                     + f"; a block ends at 63: {c['ends_at_63']}")
    lines.append(f"  longest lane pattern {cov['longest']} bits; patterns over 32 bits start at {len(cov['offsets'])} of 32 offsets"
                 f" (missing {sorted(set(range(32)) - cov['offsets'])}); 0xFF last / first byte of a chunk: {cov['ff_last']} / {cov['ff_first']}"
                 f" (both in one frame: {cov['ff_both']})")
    return "\n".join(lines)


def bits_per_block(img, quality):
    """Coded bits of a frame over its blocks in scan order (dummy blocks included): what jpeg_encode_sizes bounds by max_block_bits."""
    z, tbl = J.scan_blocks(img, quality)
    return float(J.entropy_bits(z, tbl)[1].sum()) / len(z)


def densest(mode):
    """The designed frame of a mode with the most bits per block, as (name, quality, image)."""
    return max(frames(mode), key=lambda f: bits_per_block(f[2], f[1]))


# ---- what the mosaics reach: the floors tests/test_jpeg_symbols_host.py asserts -----------------------------------------------------------
# Every (run & 15, size) of the 160 that the mosaics do NOT code, by table, each with its reason; the host test asserts that the coded
# set is exactly the complement.  Both lists are empty.  The first search alone (one value per size, 1.25 * 2^(size - 1)) misses four:
#   luma (11, 10) and (12, 10): a value of 640 at positions 12 / 13 swings the samples by 160, they clip, and the clipping codes a
#                               coefficient inside the run;
#   chroma (12, 9) and (14, 10): the same at positions 13 / 15 once Cb leaves 0..255 on the yellow-blue line.
# The sweep reaches them with values of 512..530 (256.. for size 9), which stay in range.  Size 10 is the largest an AC coefficient of
# 8-bit samples can have: |c| <= 128 * 8 = 1024 needs all 64 samples at the extremes with the basis' signs, and 1023 is the most
# the Huffman tables can code.
UNREACHED = {"luma": {}, "chroma": {}}
AC_FLOOR = {"luma": 160, "chroma": 160}          # the plain construction: 158 and 158 (146 for chroma with Y = Cr = 128 alone)
# 63 bits is the longest pattern a lane can build: three luma ZRLs (33), a 16-bit code, 10 value bits and the luma EOB (4).  The sweep
# finds it: a size-10 coefficient alone in its block behind a run of 48 or more.  The first search stops at 60 (size 7 there).
LONGEST_PATTERN = 63
