"""Writes the palette chooser's cases for tools/quantize_check.cpp: every hand-computed case of tests/quantize_cases.py with its
hand-computed answer, and the generated frames at every K of the device tests with the palette tests/quantize_ref.py gives them.

    python tools/quantize_dump_cases.py cases.bin

Format, little endian: u32 count; per case u32 name length, the name, u32 K, u32 pixels, the pixels (3 bytes each), u32 used, the 768
palette bytes.
"""
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import quantize_cases as C  # noqa: E402
import quantize_ref as Q  # noqa: E402


def cases():
    for name, frames, K, entries in C.HAND:
        yield name, frames, K, C.expected(entries)
    for name, frames in C.generated():
        for K in C.KS:
            yield f"{name}, K {K}", frames, K, Q.palette(frames, K)
        yield f"{name}, frame 0, K 16", frames[0], 16, Q.palette(frames[0], 16)


def main(path):
    blobs = []
    for name, frames, K, (pal, used) in cases():
        px = frames.reshape(-1, 3)
        tag = name.encode()
        blobs.append(struct.pack("<I", len(tag)) + tag + struct.pack("<II", K, len(px)) + px.tobytes() + struct.pack("<I", used) + pal.tobytes())
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)) + b"".join(blobs))
    print(f"{len(blobs)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
