"""CPU check of the block synchroniser the kernel rds_sync runs (sdr-j-fm_amd/csrc/fmx_rdssync.h) against the host decoder's own
(RdsGroupDecoderHost::push_bit, fmx_rdsgroups.h): the header's functions compiled for the host (tests/rdssync_check.cpp).  The syndrome by masked
popcounts against the 26-step loop on every 26-bit word and offset word; the synchroniser plus push_group against push_bit, every field of the info
after every bit, on clean and damaged streams; the kernel's walk over the bit ring in chunks of 0, 1, 25, 26, 27 and 119 bits; and the same program
once more under the address and undefined-behaviour sanitizers."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rds_streams as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rdssync_check.cpp")


def compiler():
    cc = shutil.which("g++") or shutil.which("c++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    return cc


def runner(exe):
    def run(queries, timeout=600):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True, timeout=timeout).stdout.splitlines()
        assert len(out) == len(queries), out
        return [json.loads(line) for line in out]
    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rdssync") / "rdssync_check")
    subprocess.check_call([compiler(), "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe, SRC])
    return runner(exe)


def streams():
    """name -> (bits, the paths the stream must reach)"""
    rng = np.random.default_rng(7)
    a = rs.programme(**rs.PROG_A)
    two = np.concatenate([a, a])
    s = {}
    s["clean"] = (np.concatenate([two, a]), dict(complete=30, found_a=1))
    s["payload_bit"] = (rs.flip(two, [rs.bit_index(5, 2, 7)]), dict(no_crc=1, meggitt_run=1))
    s["burst5"] = (rs.flip(two, [rs.bit_index(5, 3, 4 + k) for k in (0, 1, 3, 4)]), dict(no_crc=1, meggitt_flip=2))
    s["burst3"] = (rs.flip(two, [rs.bit_index(6, 1, 9 + k) for k in range(3)]), dict(no_crc=1, meggitt_flip=2))
    s["checkword"] = (rs.flip(two, [rs.bit_index(5, 1, 21)]), dict(no_crc=1))
    d = rs.bit_index(5, 2, 11)
    s["dropped_bit"] = (np.concatenate([two[:d], two[d + 1:]]), dict(no_crc=1, waiting_a=20, found_a=2))
    s["inserted_bit"] = (np.concatenate([two[:d], [1], two[d:]]), dict(no_crc=1, waiting_a=20, found_a=2))
    s["sync_error"] = (rs.flip(two, [rs.bit_index(5, 3, 2), rs.bit_index(6, 1, 3)]), dict(no_crc=1, no_sync=1))
    s["type_b"] = (np.concatenate([a[:4 * rs.GROUP], rs.type_b_group(), rs.type_b_group(), a[4 * rs.GROUP:]]), dict(type_b_offset=2, complete=14))
    s["pi_change"] = (np.concatenate([a, rs.programme(**rs.PROG_B), a]), dict(complete=30))
    # 4000 payload bits and more between the error counters' wraps: 96 groups, a damaged payload in every fifth
    long = np.concatenate([a] * 8)
    s["ber_wrap"] = (rs.flip(long, [rs.bit_index(g, g % 4, 3 + g % 11) for g in range(3, 96, 5)]), dict(ber_wrap=1, no_crc=10, meggitt_run=10))
    s["faulty_payload_x3"] = (np.concatenate([rs.faulty_payload()] * 3), dict(no_crc=9, no_sync=1, type_b_offset=1, meggitt_flip=1))
    s["random"] = (rng.integers(0, 2, 60000).astype(np.uint8), dict(waiting_a=50000, found_a=20, no_sync=20))
    s["random_then_clean"] = (np.concatenate([rng.integers(0, 2, 3001).astype(np.uint8), two]), dict(complete=20))
    s["empty"] = (np.zeros(0, np.uint8), {})
    return s


def query(name, bits):
    return "stream %s %s" % (name, "".join("1" if b else "0" for b in bits))


def verify(results, S):
    for (name, (bits, reach)), g in zip(S.items(), results):
        assert g["name"] == name and g["bits"] == bits.size
        assert g["field_mismatches"] == 0, (name, g["first"])
        assert g["chunk_mismatches"] == 0, name
        for k, least in reach.items():
            assert g[k] >= least, (name, k, g)


def test_syndrome_every_word(check):
    g = check(["syndrome"])[0]
    assert g["checked"] == 5 * 2 ** 26 + 2 ** 20 and g["mismatches"] == 0, g


def test_synchroniser_equals_push_bit(check):
    S = streams()
    got = check([query(n, b) for n, (b, _) in S.items()])
    verify(got, S)
    by = {g["name"]: g for g in got}
    # what the streams are for: the clean one decodes every group behind the first three blocks, each fault costs what the reference makes it cost
    assert by["clean"]["groups"] == 36 and by["clean"]["crc_errors"] == 0 and by["clean"]["pi_code"] == 0xD3A1 and by["clean"]["synchronized"] == 1
    assert by["payload_bit"]["groups"] == 23 and by["payload_bit"]["crc_errors"] == 1
    assert by["pi_change"]["pi_code"] == 0xD3A1 and by["pi_change"]["groups"] == 12 + 8 + 12
    assert by["type_b"]["groups"] == 14
    assert by["empty"]["groups"] == 0 and by["empty"]["ber_bits"] == 0
    # every path named in the header's RdsSyncCover was taken by some stream
    for k in ("waiting_a", "found_a", "no_sync", "no_crc", "complete", "meggitt_run", "meggitt_flip", "ber_wrap", "type_b_offset"):
        assert any(g[k] > 0 for g in got), k


def test_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined: a stand-alone binary, every query again."""
    exe = str(tmp_path / "rdssync_check_san")
    r = subprocess.run([compiler(), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", exe, SRC],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-2000:]
    S = streams()
    got = runner(exe)([query(n, b) for n, (b, _) in S.items()] + ["syndrome"])
    verify(got[:-1], S)
    assert got[-1]["mismatches"] == 0
