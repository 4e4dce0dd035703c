"""Carry of an emulation-prevention tile (csrc/codec/h264_ep.h): the backward scan that
k_ep_count runs per 4 KiB tile, in its serial host form, against a plain forward loop.
A stand-alone program built with AddressSanitizer and UBSan; nothing is loaded into Python."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "h264_ep.h"

using namespace sk::h264;
constexpr int kTile = 4096;

// RBSP bytes -> words, most significant byte first; exactly the words the bytes need
static std::vector<uint32_t> pack(const std::vector<uint8_t>& b) {
    std::vector<uint32_t> w((b.size() + 3) / 4, 0u);
    for (size_t i = 0; i < b.size(); i++) w[i >> 2] |= (uint32_t)b[i] << (24 - 8 * (i & 3));
    return w;
}

static int forward(const std::vector<uint8_t>& b, int t0) {
    int c = -1;
    for (int i = 0; i < t0; i++)
        if (b[i]) c = i;
    return c;
}

static int checks = 0, failures = 0;

// every tile of the buffer, with 1 lane (the serial form) and with 64 lanes run one after another
static void check(const std::vector<uint8_t>& b, const char* what) {
    const std::vector<uint32_t> w = pack(b);
    for (int t0 = 0; t0 < (int)b.size(); t0 += kTile) {
        const int want = forward(b, t0);
        // heap copy of exactly the words before the tile: a read at or past t0 / 4 is an ASan error
        std::vector<uint32_t> before(w.begin(), w.begin() + t0 / 4);
        const int got = ep_tile_carry(before.data(), t0, 0, 1, [](bool p) { return (uint64_t)p; });
        // the 64-lane form, one lane after another: ballot() hands every lane the wave's mask
        // of that step (worked out here) and checks the lane's own predicate against its bit
        std::vector<uint64_t> masks;
        for (int top = t0 / 4 - 1; top >= 0; top -= 64) {
            uint64_t m = 0;
            for (int l = 0; l < 64; l++)
                if (top - l >= 0 && before[top - l] != 0u) m |= 1ull << l;
            masks.push_back(m);
        }
        int got64 = -2;
        for (int l = 0; l < 64; l++) {
            size_t step = 0;
            bool pred_ok = true;
            const int r = ep_tile_carry(before.data(), t0, l, 64, [&](bool p) {
                const uint64_t m = masks.at(step++);
                pred_ok = pred_ok && p == (((m >> l) & 1) != 0);
                return m;
            });
            if (l == 0) got64 = r;
            if (r != got64 || !pred_ok) got64 = -3;
        }
        checks++;
        if (got != want || got64 != want) {
            failures++;
            std::printf("FAIL %s: t0 %d want %d serial %d wave %d\n", what, t0, want, got, got64);
        }
    }
    for (int q = 0; q < 4; q++) {   // byte order helper
        const uint32_t word = 0x01020304u;
        if (ep_rbsp_byte(word, q) != q + 1) { failures++; std::printf("FAIL ep_rbsp_byte\n"); }
    }
}

int main() {
    // zero runs of length 0..70 ending exactly at, one before and one after a tile boundary
    for (int run = 0; run <= 70; run++)
        for (int end = kTile - 1; end <= kTile + 1; end++) {   // the run covers [end - run, end)
            std::vector<uint8_t> b(2 * kTile + 100);
            for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)(1 + i % 255);
            for (int i = end - run; i < end; i++) b[i] = 0;
            check(b, "zero run at a boundary");
            // the same with the second boundary
            std::vector<uint8_t> c(2 * kTile + 100);
            for (size_t i = 0; i < c.size(); i++) c[i] = (uint8_t)(1 + i % 255);
            for (int i = kTile + end - run; i < kTile + end; i++) c[i] = 0;
            check(c, "zero run at the second boundary");
        }
    {   // a tile that is entirely zero (and the one after it looks back across it)
        std::vector<uint8_t> b(3 * kTile + 17, 0x55);
        std::memset(b.data() + kTile, 0, kTile);
        check(b, "all-zero tile");
        std::memset(b.data(), 0, kTile);   // nothing but zeros before tile 2: carry -1
        check(b, "all zero before");
        b[5] = 9;                          // a lone byte far back
        check(b, "lone byte");
    }
    {   // a first tile only
        std::vector<uint8_t> b(100, 7);
        check(b, "first tile");
    }
    {   // a last partial tile after two full ones, with zeros around the boundary
        std::vector<uint8_t> b(2 * kTile + 3, 0);
        b[kTile - 7] = 1;
        b[2 * kTile + 1] = 1;
        check(b, "last partial tile");
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
"""


def test_tile_carry_matches_forward_loop(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler")
    src = tmp_path / "ep_carry.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ep_carry"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'csrc' / 'codec'}", str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 failures" in r.stdout
