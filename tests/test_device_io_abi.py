"""Device encryption / decryption without a GPU: the four entries of include/fbs_exec.h are declared, exported and bound, the
facade takes the device path by default, and the ChaCha20 block function the host and the kernels share (csrc/fbs_chacha.hpp)
is ChaCha20: RFC 7539 section 2.3.2, and block-by-block agreement with a Python ChaCha20 under the 64-bit-counter layout."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe_fbs_map_amd", "csrc")
ENTRIES = ("fbs_encrypt_dev", "fbs_encrypt_fresh_dev", "fbs_decrypt_dev", "fbs_eval_messages")
M32 = 0xFFFFFFFF


def test_entries_are_declared_exported_and_bound():
    from tests.test_capi_symbols import declared_symbols
    from tfhe_fbs_map_amd import ExecConfig, _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
    assert ExecConfig().device_io is True


# ---- a Python ChaCha20, original layout: words 12-13 the 64-bit block counter, 14-15 the 64-bit stream id -----------------
def _rol(v, s):
    return ((v << s) | (v >> (32 - s))) & M32


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rol(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rol(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rol(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rol(x[b] ^ x[c], 7)


def chacha_block(key, stream, counter):
    """8 little-endian 64-bit words of block `counter` of stream `stream` under the 8-word key"""
    st = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *key, counter & M32, counter >> 32, stream & M32, stream >> 32]
    x = list(st)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    y = [(a + b) & M32 for a, b in zip(x, st)]
    return [y[2 * i] | (y[2 * i + 1] << 32) for i in range(8)]


def irwin_hall(w, sigma):
    s = -6 * M32 + sum((v & M32) + (v >> 32) for v in w)
    return (s * sigma + (1 << 31)) >> 32


RFC_KEY = [int.from_bytes(bytes(range(4 * i, 4 * i + 4)), "little") for i in range(8)]   # 00:01:02 .. 1f
RFC_COUNTER = 1 | (0x09000000 << 32)   # block count 1, nonce 00:00:00:09:00:00:00:4a:00:00:00:00
RFC_STREAM = 0x4A000000
RFC_BLOCK = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                          "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "fbs_chacha.hpp"
// argv: 8 key words, stream, first block, blocks, sigma -> the words of each block, then irwin_hall_sample of words 0..5 of each
int main(int argc, char **argv) {
    if (argc != 13) return 2;
    uint32_t key[8];
    for (int i = 0; i < 8; i++) key[i] = (uint32_t)strtoull(argv[1 + i], nullptr, 0);
    const uint64_t stream = strtoull(argv[9], nullptr, 0), first = strtoull(argv[10], nullptr, 0), n = strtoull(argv[11], nullptr, 0);
    const uint64_t sigma = strtoull(argv[12], nullptr, 0);
    for (uint64_t b = first; b < first + n; b++) {
        uint64_t w[8];
        fbs::chacha_block(key, stream, b, w);
        for (int i = 0; i < 8; i++) printf("%" PRIu64 " ", w[i]);
        printf("%" PRId64 "\n", fbs::irwin_hall_sample(w, sigma));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("chacha")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def run_driver(driver, key, stream, first, n, sigma=0):
    out = subprocess.check_output([driver, *map(str, key), str(stream), str(first), str(n), str(sigma)], text=True)
    rows = [list(map(int, line.split())) for line in out.splitlines()]
    return [r[:8] for r in rows], [r[8] for r in rows]


def test_python_chacha_is_rfc7539():
    words = chacha_block(RFC_KEY, RFC_STREAM, RFC_COUNTER)
    assert b"".join(w.to_bytes(8, "little") for w in words) == RFC_BLOCK


def test_header_block_function_is_rfc7539(driver):
    (words,), _ = run_driver(driver, RFC_KEY, RFC_STREAM, RFC_COUNTER, 1)
    assert b"".join(w.to_bytes(8, "little") for w in words) == RFC_BLOCK


def test_header_matches_python_block_by_block(driver):
    """What rand_words reads: word j of a stream is word j % 8 of block j / 8; encryption streams carry domain 7 in the top byte,
    noise streams domain 8, and the 64-bit block counter runs past 2^32."""
    seed = 0x0123456789ABCDEF
    key = [seed & M32, seed >> 32, 0x2D736266, 0x63657865, 0x646D612D, 0x7866672D, 0x2D303539, 0x3179656B]
    for stream, first in (((7 << 56) | 12345, 0), ((8 << 56) | (1 << 55) | 3, 0), ((7 << 56) | (2**55 - 1), (1 << 32) - 2)):
        blocks, noise = run_driver(driver, key, stream, first, 5, sigma=0x3FFFFFF)
        flat = [w for blk in blocks for w in blk]
        for j in range(len(flat)):
            assert flat[j] == chacha_block(key, stream, first + j // 8)[j % 8]
        for blk, got in zip(blocks, noise):
            assert got == irwin_hall(blk[:6], 0x3FFFFFF)
    _, noise = run_driver(driver, key, 7 << 56, 0, 3, sigma=(1 << 46) - 1)   # the largest sigma a residue can be: 128-bit products
    assert noise == [irwin_hall(chacha_block(key, 7 << 56, b)[:6], (1 << 46) - 1) for b in range(3)]
