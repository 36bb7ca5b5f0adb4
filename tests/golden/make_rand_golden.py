#!/usr/bin/env python3
"""Write chacha20_blocks.json: single ChaCha20 blocks from `openssl enc -chacha20`, the independent reference of
tests/test_rand_cpu.py.

OpenSSL's 16-byte -iv is LE32(block counter) || 12-byte nonce; encrypting 64 zero bytes yields the key stream block.
Every triple records ONE block: OpenSSL carries a counter overflow into the nonce, RFC 8439 does not, so nothing here
crosses 2^32.  The RFC 8439 section 2.3.2 block is one of the cases (and is checked against the RFC's printed bytes
here, before anything is written)."""
import json
import os
import struct
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))

RFC_HEAD = "10f1e7e4d13b5915500fdd1fa32071c4"

CASES = [
    # (name, key, nonce (12 bytes), counter)
    ("rfc8439_2_3_2", bytes(range(32)), bytes.fromhex("000000090000004a00000000"), 1),
    ("zero_key_counter_0", bytes(32), bytes(12), 0),
    ("zero_key_counter_max", bytes(32), bytes(12), 0xFFFFFFFF),
    ("ones_key_counter_0", b"\xff" * 32, bytes(12), 0),
    ("ones_key_nonce_ones_counter_max", b"\xff" * 32, b"\xff" * 12, 0xFFFFFFFF),
    ("nonce_every_byte_set", bytes((37 * i + 11) & 0xFF for i in range(32)),
     bytes.fromhex("0102030405060708090a0b0c"), 7),
    ("counter_max_minus_1", bytes((37 * i + 11) & 0xFF for i in range(32)),
     bytes.fromhex("01030000ffffffffffffffff"), 0xFFFFFFFE),
]


def openssl_block(key, nonce, counter):
    iv = struct.pack("<I", counter) + nonce
    out = subprocess.run(["openssl", "enc", "-chacha20", "-K", key.hex(), "-iv", iv.hex()], input=bytes(64),
                         capture_output=True, check=True).stdout
    assert len(out) == 64
    return out


def main():
    cases = []
    for name, key, nonce, counter in CASES:
        blk = openssl_block(key, nonce, counter)
        if name == "rfc8439_2_3_2":
            assert blk.hex().startswith(RFC_HEAD), blk.hex()
        cases.append(dict(name=name, key=key.hex(), nonce=nonce.hex(), counter=counter, block=blk.hex()))
    version = subprocess.run(["openssl", "version"], capture_output=True, text=True).stdout.strip()
    with open(os.path.join(HERE, "chacha20_blocks.json"), "w") as f:
        json.dump(dict(source="openssl enc -chacha20, -iv = LE32(counter) || nonce, 64 zero bytes in; " + version,
                       cases=cases), f, indent=1)
        f.write("\n")
    print("wrote chacha20_blocks.json: %d blocks" % len(cases))


if __name__ == "__main__":
    main()
