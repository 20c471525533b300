"""Writes the frames of tests/gif_cases.py with the records tests/gif_ref.py gives them as one binary file for tools/gif_lzw_check.cpp:
a count, then per case a name (length, bytes), K, h, w, the delay, the record's length (all uint32, little endian), the h w indices
and the record.

    python tools/gif_lzw_dump_cases.py cases.bin
"""
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import gif_cases as C  # noqa: E402
import gif_ref as G  # noqa: E402


def main(path):
    cases = C.cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for i, (name, K, index) in enumerate(cases):
            delay = (7 * i + 1) % 65536 if i % 5 else 65535
            rec = G.record(index, K, delay)
            h, w = index.shape
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<5I", K, h, w, delay, len(rec)) + index.tobytes() + rec)
    print(f"{len(cases)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
