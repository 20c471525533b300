"""The files of the PNG decode tests: the smallest that reach every rule of tests/png_decode_ref.py.
sound() -> [Case]: files the decoder takes, with the frame they hold; damaged() -> [Case]: one per status of the decoder, with the
status.  Host only, deterministic, built once.  Not a test module."""
import functools
import os
import zlib
from dataclasses import dataclass

import numpy as np

import png_decode_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png")
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}
BAND = ref.BAND


@dataclass
class Case:
    name: str
    data: bytes                 # the file
    h: int
    w: int
    c: int
    pixels: object = None       # uint8 [h,w,c] of a sound file built here; None for a fixture (Pillow says) and for a damaged file
    status: int = 0             # what the decoder answers
    about: str = ""


def noise(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def gradient(h, w, c, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    g = np.stack([(3 * x + (k + 1) * y + 40 * k) for k in range(c)], 2) + rng.integers(-2, 3, (h, w, c))
    return (g & 255).astype(np.uint8)


def flat(h, w, c):
    """An object on black: long runs of zeros."""
    px = gradient(h, w, c, 5)
    px[:, : w // 2] = 0
    px[h // 2:] = 0
    return px


def deflate(data, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if flush_at is None:
        return co.compress(data) + co.flush()
    return co.compress(data[:flush_at]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(data[flush_at:]) + co.flush()


def mixed_filters(h):
    return [(3 * y + 1) % 5 for y in range(h)]


def file_of(px, filters, **how):
    h, w, c = px.shape
    return ref.png_file(h, w, COLOUR_TYPE[c], deflate(ref.filter_rows(px, filters), **how))


def case(name, px, filters, about="", **how):
    h, w, c = px.shape
    return Case(name, file_of(px, filters, **how), h, w, c, px, 0, about)


CL_LENS = [4] * 13 + [5] * 6           # a complete code-length code with every symbol: 13 / 16 + 6 / 32


def hand_block(bw, final, ll_lens, d_lens, tokens, items=None):
    """One dynamic block: the lengths spelled by ``items`` (default: one by one), then the tokens and the end-of-block code."""
    ref.put_dynamic_header(bw, final, ll_lens, d_lens, CL_LENS, list(ll_lens) + list(d_lens) if items is None else items)
    ref.put_tokens(bw, tokens, ref.canonical(ll_lens), ref.canonical(d_lens))


def hand_file(filtered, h, w, c, blocks):
    """A file whose zlib stream is the dynamic ``blocks`` [(ll_lens, d_lens, tokens, items)], which must spell ``filtered``."""
    bw = ref.BitWriter()
    for i, blk in enumerate(blocks):
        hand_block(bw, int(i == len(blocks) - 1), *blk)
    return ref.png_file(h, w, COLOUR_TYPE[c], ref.zlib_wrap(bw.done(), filtered))


def tokens_to_bytes(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def lens_of(n, pairs):
    lens = [0] * n
    for s, ln in pairs:
        lens[s] = ln
    return lens


def grey_row_case(name, tokens, blocks_of, about):
    """A grey one-row file whose filtered stream is what ``tokens`` spell (its first byte is the filter)."""
    filtered = tokens_to_bytes(tokens)
    w = len(filtered) - 1
    px, status = ref.unfilter(filtered, 1, w, 1)
    assert status == 0
    return Case(name, hand_file(filtered, 1, w, 1, blocks_of), 1, w, 1, px, 0, about)


def hand_cases():
    out = []
    # a 15-bit code: lengths 1..14 for the literals 1..14, 15 for literal 15 and the end of block.  The row's filter is Sub (1).
    ll = lens_of(257, [(s, s) for s in range(1, 15)] + [(15, 15), (256, 15)])
    toks = [1, 15, 14, 3, 15, 2, 9, 15]
    out.append(grey_row_case("hand_15bit", toks, [(ll, [1, 1], toks, None)], "a code of 15 bits"))
    # repeat codes across the boundary between the literal/length and the distance lengths
    ll = lens_of(259, [(0, 2), (1, 2), (256, 2), (257, 3), (258, 3)])
    toks = [0, 1, 1, 0, (3, 2), (4, 1), 1]
    items = [2, 2, (18, 127), (18, 105), 2, 3, (16, 3), 3, 3, 3]           # the 16 gives symbol 258 and five of the eight distance lengths
    out.append(grey_row_case("hand_repeat16", toks, [(ll, [3] * 8, toks, items)], "16 across HLIT"))
    ll = lens_of(260, [(1, 1), (256, 1)])
    toks = [1, 1, 1, 1]
    items = [0, 1, (18, 127), (18, 105), 1, (17, 3), 1]                 # the 17 gives three literal/length zeros and three distance zeros
    out.append(grey_row_case("hand_repeat17", toks, [(ll, [0, 0, 0, 1], toks, items)], "17 across HLIT"))
    ll = lens_of(265, [(1, 1), (256, 1)])
    items = [0, 1, (18, 127), (18, 105), 1, (18, 2), 1]                 # the 18 gives eight literal/length zeros and five distance zeros
    out.append(grey_row_case("hand_repeat18", toks, [(ll, [0] * 5 + [1], toks, items)], "18 across HLIT"))
    # a single one-bit distance code
    ll = lens_of(258, [(0, 2), (7, 2), (256, 2), (257, 2)])
    toks = [0, 7, (3, 1), 0, (3, 1)]
    out.append(grey_row_case("hand_one_distance", toks, [(ll, [1], toks, None)], "one distance code of one bit"))
    # length symbol 285, the length symbols with 5 extra bits at their largest extra, distance symbol 29 with 13 extra bits
    rng = np.random.default_rng(11)
    lits = [0] + rng.integers(0, 256, 30999).tolist()
    toks = lits + [(258, 24577), (257, 30000), (162, 8192), (258, 32768 - 2000)]
    ll = lens_of(286, [(s, 9) for s in range(256)] + [(256, 2), (281, 3), (284, 4), (285, 4)])
    d = lens_of(30, [(25, 1), (29, 1)])
    out.append(grey_row_case("hand_far", toks, [(ll, d, toks, None)], "symbols 281, 284, 285 and distance symbol 29"))
    # two dynamic blocks and an empty one between them
    ll = lens_of(257, [(0, 1), (256, 1)])
    out.append(grey_row_case("hand_blocks", [0, 0, 0], [(ll, [1], [0, 0], None), (ll, [1], [], None), (ll, [1], [0], None)], "an empty block"))
    return out


def window_case():
    """Grey 2 x 32767 under filter 0 with two identical noise rows: the filtered stream has period 32768.  zlib itself never reaches
    further back than 32768 - 262, so the stream is spelled by hand in the fixed code: 32768 literals, then matches at distance 32768."""
    row = noise(1, 32767, 1, 3)
    px = np.concatenate([row, row], 0)
    filtered = ref.filter_rows(px, [0, 0])
    toks = list(filtered[:32768]) + [(258, 32768)] * 126 + [(257, 32768), (3, 32768)]
    assert tokens_to_bytes(toks) == filtered
    bw = ref.BitWriter().bits(1, 1).bits(1, 2)
    ref.put_tokens(bw, toks, ref.canonical(ref.FIXED_LL), ref.canonical(ref.FIXED_D))
    return Case("window_32768", ref.png_file(2, 32767, 0, ref.zlib_wrap(bw.done(), filtered)), 2, 32767, 1, px, 0, "distance 32768")


def paeth_ties():
    """Grey 2 x 6: the pixels (1, 1), (1, 3) and (1, 5) see pa = pb < pc, pa = pc < pb and pb = pc < pa."""
    return np.array([[10, 13, 10, 12, 10, 6], [13, 77, 6, 77, 12, 77]], np.uint8).reshape(2, 6, 1)


def rechunk(data, sizes):
    """The file ``data`` (one IDAT) with its stream cut into IDATs of ``sizes`` (cycled; 0 gives an empty chunk), the rest in the last."""
    p = ref_parse_stream(data)
    pieces, at, k = [], 0, 0
    while at < len(p):
        n = sizes[k % len(sizes)]
        pieces.append(p[at:at + n])
        at += n
        k += 1
    return pieces


def ref_parse_stream(data):
    """The joined IDAT payloads of a file built by ref.png_file."""
    at, out = 8, b""
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], "big")
        if data[at + 4:at + 8] == b"IDAT":
            out += data[at + 8:at + 8 + n]
        at += 12 + n
    return out


@functools.lru_cache(maxsize=None)
def sound():
    out = []
    for c, mode in ((1, "L"), (3, "RGB"), (4, "RGBA")):
        out.append(case(f"1x1_{mode}", noise(1, 1, c, c), [4]))
    for w, c in ((1, 1), (1, 3), (5, 1), (7, 1)):
        out.append(case(f"rowbytes_{w * c}", noise(3, w, c, 20 + w * c), [1, 4, 3], "row bytes off the 4-byte grid"))
    for h in (BAND - 1, BAND, BAND + 1, 2 * BAND + 1):
        out.append(case(f"height_{h}", gradient(h, 5, 3, h), mixed_filters(h), "around the unfilter's band"))
    for ft in range(5):
        out.append(case(f"filter_{ft}", noise(7, 9, 3, 30 + ft), [ft] * 7, "one filter on every row, the first included"))
    out.append(case("filter_mixed_rgba", noise(11, 6, 4, 40), mixed_filters(11)))
    out.append(case("filter_average_noise", noise(5, 33, 1, 41), [3] * 5, "9-bit sums"))
    out.append(case("paeth_ties", paeth_ties(), [4, 4], "every tie of Paeth"))
    g = gradient(40, 33, 3, 50)
    out.append(case("zlib_stored", g, mixed_filters(40), "BTYPE 0", level=0))
    out.append(case("zlib_stored_two", gradient(150, 150, 3, 51), mixed_filters(150), "more than 65535 bytes: two stored blocks", level=0))
    out.append(case("zlib_fixed", g, mixed_filters(40), "BTYPE 1", strategy=zlib.Z_FIXED))
    out.append(case("zlib_huffman_only", g, mixed_filters(40), "no matches", strategy=zlib.Z_HUFFMAN_ONLY))
    out.append(case("zlib_rle", flat(40, 33, 3), [0] * 40, "distance 1, overlapping copies up to 258", strategy=zlib.Z_RLE))
    out.append(case("zlib_default", g, mixed_filters(40), "BTYPE 2"))
    out.append(case("zlib_level9", flat(40, 33, 4), mixed_filters(40), level=9))
    out.append(case("zlib_wbits9", g, mixed_filters(40), "header 18 95", wbits=9))
    out.append(case("zlib_sync_flush", g, mixed_filters(40), "an empty stored block between Huffman blocks", flush_at=2000))
    out.append(window_case())
    out += hand_cases()
    base = file_of(g, mixed_filters(40))
    n = len(ref_parse_stream(base))
    for name, pieces, before, after in (
            ("idat_1_rest", rechunk(base, [1, n]), (), ()),
            ("idat_every_byte", rechunk(base, [1]), (), ()),
            ("idat_empty_between", [b""] + rechunk(base, [0, 1, 0, 700]) + [b""], (), ()),
            ("idat_ancillary", rechunk(base, [900]), ((b"tEXt", b"Title\0designed"), (b"pHYs", bytes(9))), ((b"tIME", bytes(7)),))):
        out.append(Case(name, ref.png_file(40, 33, 2, pieces, before, after), 40, 33, 3, g, 0, "IDAT splitting"))
    for name, c in (("view_800.png", 3), ("conv_1.png", 4)):
        with open(os.path.join(GOLDEN, name), "rb") as f:
            data = f.read()
        w, h = int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big")
        out.append(Case("fixture_" + name, data, h, w, c, None, 0, "the modelled project's own file"))
    return tuple(out)


def fixed_stream(tokens_bits):
    """A final fixed block whose body is written by ``tokens_bits(bw, ll, d)``; no end-of-block code is added."""
    bw = ref.BitWriter().bits(1, 1).bits(1, 2)
    tokens_bits(bw, ref.canonical(ref.FIXED_LL), ref.canonical(ref.FIXED_D))
    return bw.done()


def dynamic_stream(ll_lens, d_lens, tokens, items=None, hlit=None):
    bw = ref.BitWriter()
    if hlit is None:
        hand_block(bw, 1, ll_lens, d_lens, tokens, items)
    else:                       # a header that claims `hlit` literal/length codes, and nothing behind HCLEN's lengths that matters
        bw.bits(1, 1).bits(2, 2).bits(hlit - 257, 5).bits(0, 5).bits(15, 4)
        for _ in range(19):
            bw.bits(4, 3)
    return bw.done()


@functools.lru_cache(maxsize=None)
def damaged():
    px = gradient(2, 4, 1, 60)                  # grey 2 x 4: a filtered stream of 10 bytes
    filtered = ref.filter_rows(px, [1, 2])
    good = deflate(filtered)                    # 78 9c, a fixed block, the Adler-32
    stored = deflate(filtered, level=0)
    adler = good[-4:]
    out = []

    def add(name, stream, status, about, h=2, w=4, c=1):
        out.append(Case(name, ref.png_file(h, w, COLOUR_TYPE[c], stream), h, w, c, None, status, about))

    ll2 = lens_of(257, [(0, 1), (256, 1)])
    full = ref.zlib_wrap(dynamic_stream(ll2, [1], [0] * 10), bytes(10))
    add("cut_at_zlib_header", good[:2], ref.TRUNCATED, "nothing behind the zlib header")
    add("cut_in_dynamic_header", full[:9], ref.TRUNCATED, "the stream ends inside the code lengths")
    add("cut_in_stored", stored[:10], ref.TRUNCATED, "the stream ends inside a stored block")
    add("cut_before_adler_end", good[:-1], ref.TRUNCATED, "one byte of the Adler-32 is missing")
    add("block_type_3", b"\x78\x01\x07" + adler, ref.BLOCK_TYPE, "BTYPE 3")
    add("stored_len", stored[:5] + bytes([stored[5] ^ 1]) + stored[6:], ref.STORED_LEN, "NLEN is not ~LEN")
    add("oversubscribed", ref.zlib_wrap(dynamic_stream(lens_of(257, [(0, 1), (1, 1), (256, 1)]), [1], []), filtered), ref.OVERSUBSCRIBED, "three codes of one bit")
    add("incomplete", ref.zlib_wrap(dynamic_stream(lens_of(257, [(0, 2), (1, 2), (256, 2)]), [1], []), filtered), ref.INCOMPLETE, "three codes of two bits")
    add("repeat_first", ref.zlib_wrap(dynamic_stream(ll2, [1], [], [(16, 0)]), filtered), ref.REPEAT, "16 with nothing to repeat")
    add("repeat_past_end", ref.zlib_wrap(dynamic_stream(ll2, [1], [], [1, (18, 127), (18, 110)]), filtered), ref.REPEAT, "18 past HLIT + HDIST")
    noend = ref.BitWriter()
    ref.put_dynamic_header(noend, 1, lens_of(257, [(0, 1), (1, 1)]), [1], CL_LENS, [1, 1, (18, 127), (18, 107)])
    add("no_end_of_block", ref.zlib_wrap(noend.done() + bytes(4), filtered), ref.NO_END_OF_BLOCK, "symbol 256 without a code")
    add("length_symbol_286", ref.zlib_wrap(fixed_stream(lambda bw, ll, d: bw.code(*ll[1]).code(*ll[286])) + bytes(4), filtered), ref.BAD_SYMBOL, "length symbol 286")
    add("distance_symbol_30", ref.zlib_wrap(fixed_stream(lambda bw, ll, d: bw.code(*ll[1]).code(*ll[257]).code(*d[30])) + bytes(4), filtered), ref.BAD_SYMBOL,
        "distance symbol 30")
    add("far_distance", ref.zlib_wrap(fixed_stream(lambda bw, ll, d: bw.code(*ll[1]).code(*ll[257]).code(*d[1])) + bytes(4), filtered), ref.FAR_DISTANCE,
        "distance 2 behind one byte")
    add("too_much", deflate(ref.filter_rows(gradient(3, 4, 1, 61), [1, 2, 0])), ref.TOO_MUCH, "three rows in a file of two")
    add("too_little", good, ref.TOO_LITTLE, "two rows in a file of three", h=3)
    add("trailing_before_adler", good[:-4] + b"\0" + adler, ref.TRAILING, "a byte between the final block and the Adler-32")
    add("trailing_behind_adler", good + b"\0", ref.TRAILING, "a byte behind the Adler-32")
    add("adler", good[:-1] + bytes([good[-1] ^ 1]), ref.ADLER, "a flipped bit in the Adler-32")
    bad_filter = bytes([5]) + filtered[1:]
    add("filter_5", deflate(bad_filter), ref.FILTER, "a filter byte of 5")
    lone = ref.BitWriter()
    ll3 = lens_of(258, [(0, 2), (1, 2), (256, 2), (257, 2)])
    ref.put_dynamic_header(lone, 1, ll3, [1], CL_LENS, ll3 + [1])
    lone.code(*ref.canonical(ll3)[1]).code(*ref.canonical(ll3)[257]).bits(1, 1)          # the distance code's other bit
    add("unused_code", ref.zlib_wrap(lone.done() + bytes(4), filtered), ref.UNUSED_CODE, "the bit that the one distance code leaves free")
    add("too_many_symbols", ref.zlib_wrap(dynamic_stream(None, None, None, hlit=287) + bytes(8), filtered), ref.TOO_MANY_SYMBOLS, "HLIT of 287")
    return tuple(out)
