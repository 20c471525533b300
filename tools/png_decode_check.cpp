// The inflate and unfilter cores of the PNG decoder (csrc/png_inflate.h) on the CPU: a stand-alone program for a sanitised build.
//
//   python tools/png_decode_dump_cases.py cases.bin         # every sound and damaged file of tests/png_decode_cases.py
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/png_decode_check.cpp -o png_decode_check
//   ./png_decode_check cases.bin
//
// Every case runs the way the device runs it - 64 lanes, the stream seen through a 1 KiB stage that is refilled before every step, the
// window in a 64 KiB ring - and once more with the whole stream visible; both must give the case's status and, for a sound file, its
// pixels in the file's channels and in 3.  Every buffer is a heap block of exactly its size, so that a read or a write outside it stops
// the program.  Exit status 0: every case agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../applied-image-processing_amd/csrc/png_inflate.h"

using namespace adain;

namespace {

struct Case {
    std::string name;
    int h, w, c, status;
    std::vector<uint8_t> stream, pixels;
};

bool read_u32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

bool read_cases(const char* path, std::vector<Case>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint32_t count;
    if (!read_u32(f, &count)) return false;
    for (uint32_t i = 0; i < count; ++i) {
        Case c;
        uint32_t n, v[4], stream, pixels;
        if (!read_u32(f, &n)) return false;
        c.name.resize(n);
        if (n && fread(&c.name[0], 1, n, f) != n) return false;
        if (fread(v, 4, 4, f) != 4 || !read_u32(f, &stream) || !read_u32(f, &pixels)) return false;
        c.h = (int)v[0], c.w = (int)v[1], c.c = (int)v[2], c.status = (int)v[3];
        c.stream.resize(stream), c.pixels.resize(pixels);
        if (stream && fread(c.stream.data(), 1, stream, f) != stream) return false;
        if (pixels && fread(c.pixels.data(), 1, pixels, f) != pixels) return false;
        out->push_back(c);
    }
    fclose(f);
    return true;
}

// The inflate kernel's loop with the lanes one after the other -> status; filt: exactly S bytes
int inflate(const uint8_t* in, size_t in_len, uint8_t* filt, uint64_t S, bool staged) {
    constexpr int LANES = 64;
    pngd::State* st = new pngd::State;
    pngd::Tables* tb = new pngd::Tables;
    uint8_t* ring = (uint8_t*)malloc(pngd::RING);
    uint8_t* stage = (uint8_t*)malloc(pngd::STAGE);
    pngd::AdlerPart acc[LANES] = {};
    pngd::start(*st, in_len, S);
    const uint64_t steps = pngd::max_steps(in_len);
    bool more = st->status == 0;
    for (uint64_t i = 0; more && i < steps; ++i) {
        if (staged) {
            for (int k = 0; k < pngd::STAGE; ++k) stage[k] = st->next + k < in_len ? in[st->next + k] : 0;
            pngd::step(*st, *tb, stage, true);
        } else
            pngd::step(*st, *tb, in, false);
        if (st->status == 0) {
            for (int l = 0; l < LANES; ++l) {
                if (st->stored_len) pngd::write_stored(*st, l, LANES, in, ring, filt, acc[l]);
                pngd::write_literals(*st, l, LANES, ring, filt, acc[l]);
            }
            for (int k = 0; k < st->count; ++k)
                if (pngd::is_match(*st, k))
                    for (int l = 0; l < LANES; ++l) pngd::write_match(*st, k, l, LANES, ring, filt, acc[l]);
            for (int l = 0; l < LANES; ++l) pngd::settle(acc[l]);
        }
        more = st->status == 0 && st->mode != pngd::MODE_DONE;
    }
    uint64_t a = 0, b = 0;
    for (int l = 0; l < LANES; ++l) a += acc[l].a % pngd::ADLER_MOD, b += acc[l].b % pngd::ADLER_MOD;
    int status = st->status;
    if (!status && st->mode != pngd::MODE_DONE) status = ADAIN_PNGD_TRUNCATED;
    if (!status && pngd::adler_of(a, b, S) != st->adler) status = ADAIN_PNGD_ADLER;
    delete st;
    delete tb;
    free(ring), free(stage);
    return status;
}

int decode(const Case& c, int c_out, bool staged, std::vector<uint8_t>* pixels) {
    const uint64_t S = ((uint64_t)c.w * c.c + 1) * c.h;
    uint8_t* in = (uint8_t*)malloc(c.stream.size() ? c.stream.size() : 1);
    memcpy(in, c.stream.data(), c.stream.size());
    uint8_t* filt = (uint8_t*)malloc(S);
    memset(filt, 0xa5, S);
    int status = inflate(in, c.stream.size(), filt, S, staged);
    if (!status) {
        const size_t bytes = (size_t)c.h * c.w * c_out;
        uint8_t* out = (uint8_t*)malloc(bytes);
        bool bad = false;
        for (int r0 = 0; r0 < c.h; r0 += pngd::BAND) bad |= pngd::unfilter_band<64>(filt, c.h, c.w, c.c, c_out, r0, out, 0);
        if (bad) status = ADAIN_PNGD_FILTER;
        pixels->assign(out, out + bytes);
        free(out);
    }
    free(in), free(filt);
    return status;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    std::vector<Case> cases;
    if (!read_cases(argv[1], &cases)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int wrong = 0, sound = 0, damaged = 0;
    for (const Case& c : cases) {
        (c.status ? damaged : sound)++;
        for (int staged = 0; staged < 2; ++staged)
            for (int c_out : {c.c, 3}) {
                std::vector<uint8_t> px;
                const int status = decode(c, c_out, staged != 0, &px);
                bool ok = status == c.status;
                if (ok && !status) {
                    std::vector<uint8_t> want;
                    if (c_out == c.c) want = c.pixels;
                    else
                        for (size_t i = 0; i < (size_t)c.h * c.w; ++i)
                            for (int k = 0; k < 3; ++k) want.push_back(c.pixels[i * c.c + (c.c == 1 ? 0 : k)]);
                    ok = px == want;
                }
                if (!ok) {
                    ++wrong;
                    printf("WRONG %s (c_out %d, %s): status %d, expected %d\n", c.name.c_str(), c_out, staged ? "staged" : "whole", status, c.status);
                }
            }
    }
    printf("%d sound and %d damaged cases, each staged and whole, in the file's channels and in 3: %d wrong\n", sound, damaged, wrong);
    return wrong ? 1 : 0;
}
