"""Chunked emulation prevention (csrc/codec/h264_ep.h, ep_chunk / ep_lane): the step that
k_slice_pack runs per 8 KiB chunk of a NAL, with the last non-zero byte index and the
insertion count carried from chunk to chunk, against a plain serial emulation-prevention
loop over the whole buffer. A stand-alone program built with AddressSanitizer and UBSan;
nothing is loaded into Python."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "h264_ep.h"

using namespace sk::h264;
constexpr int kChunk = 8192;   // k_slice_pack's kPackChunk

// 7.4.1 as the bitstream writer does it: a 0x03 after two zeros that a byte <= 3 follows
static std::vector<int> serial(const std::vector<uint8_t>& b) {
    std::vector<int> pos;
    int zeros = 0;
    for (int i = 0; i < (int)b.size(); i++) {
        if (zeros >= 2 && b[i] <= 3) {
            pos.push_back(i);
            zeros = 0;
        }
        zeros = b[i] == 0 ? zeros + 1 : 0;
    }
    return pos;
}

static int checks = 0, failures = 0;

static void check(const std::vector<uint8_t>& b, int chunk, const char* what) {
    const std::vector<int> want = serial(b);
    std::vector<int> got;
    EpState st;
    for (int i0 = 0; i0 < (int)b.size(); i0 += chunk) {
        const int n = std::min(chunk, (int)b.size() - i0);
        // heap copies of exactly the chunk's bytes and of room for n positions: a read or a
        // write outside them is an ASan error
        std::vector<uint8_t> bytes(b.begin() + i0, b.begin() + i0 + n);
        std::vector<int> pos(n);
        const int before = st.ins;
        const int k = ep_chunk(bytes.data(), i0, n, st, pos.data());
        if (st.ins != before + k) { failures++; std::printf("FAIL %s: insertion count\n", what); }
        got.insert(got.end(), pos.begin(), pos.begin() + k);
        int last = -1;   // the carried state against a forward loop
        for (int i = 0; i < i0 + n; i++)
            if (b[i]) last = i;
        if (st.last_nz != last) { failures++; std::printf("FAIL %s: last_nz %d want %d\n", what, st.last_nz, last); }
    }
    checks++;
    if (got != want) {
        failures++;
        std::printf("FAIL %s: chunk %d: %zu insertions, want %zu\n", what, chunk, got.size(), want.size());
    }
}

static std::vector<uint8_t> filled(size_t n) {
    std::vector<uint8_t> b(n);
    for (size_t i = 0; i < n; i++) b[i] = (uint8_t)(1 + i % 255);
    return b;
}

int main() {
    // zero runs of length 0..70 ending one byte before, at, and one byte after the first and
    // the second chunk boundary; the byte after the run is 1 (<= 3: insertion) or 9 (none)
    for (int run = 0; run <= 70; run++)
        for (int bound = 1; bound <= 2; bound++)
            for (int end = bound * kChunk - 1; end <= bound * kChunk + 1; end++)
                for (int next : {1, 9}) {
                    std::vector<uint8_t> b = filled(2 * kChunk + 100);
                    for (int i = end - run; i < end; i++) b[i] = 0;
                    b[end] = (uint8_t)next;
                    check(b, kChunk, "zero run at a boundary");
                }
    {   // a chunk of nothing but zeros, between two others, then with zeros before it too
        std::vector<uint8_t> b = filled(3 * kChunk + 17);
        std::memset(b.data() + kChunk, 0, kChunk);
        check(b, kChunk, "all-zero chunk");
        std::memset(b.data(), 0, kChunk);
        check(b, kChunk, "all zero from the start");
        b[5] = 9;
        check(b, kChunk, "lone byte");
    }
    {   // a first chunk only, shorter than one lane, and an empty tail lane
        check(filled(100), kChunk, "first chunk");
        std::vector<uint8_t> b(7, 0);
        check(b, kChunk, "seven zeros");
        b.assign(16, 0);
        check(b, kChunk, "one lane of zeros");
    }
    {   // a last partial chunk after two full ones, zeros around the boundary, ending in zeros
        std::vector<uint8_t> b(2 * kChunk + 3, 0);
        b[kChunk - 7] = 1;
        b[2 * kChunk + 1] = 1;
        check(b, kChunk, "last partial chunk");
        b[2 * kChunk + 1] = 0;
        check(b, kChunk, "ending in zeros");
    }
    {   // pseudo-random bytes, mostly small; also in chunks that are no multiple of a lane
        std::vector<uint8_t> b(3 * kChunk + 1234);
        uint32_t x = 12345;
        for (auto& v : b) {
            x = x * 1664525u + 1013904223u;
            v = (x >> 24) < 200 ? 0 : (uint8_t)((x >> 16) & 7);
        }
        check(b, kChunk, "random");
        check(b, 16384, "random, 16 KiB chunks");
        check(b, 1000, "random, chunks of 1000");
        check(b, 1, "random, chunks of one byte");
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
"""


def test_chunked_ep_matches_serial_loop(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler")
    src = tmp_path / "ep_chunks.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ep_chunks"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'csrc' / 'codec'}", str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 failures" in r.stdout
