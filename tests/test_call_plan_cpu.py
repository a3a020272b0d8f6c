"""CPU check of how a call becomes launches (sdr-j-fm_amd/csrc/fmx_plan.h): the pieces a call is made in, stage A's split in time, stage B's form and
its two channel groups -- the header's own functions, compiled for the host (tests/call_plan_check.cpp), against the values the comments, the GPU suite
and INTEGRATION.md quote."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDS_BLK = 32000
BENCH_N = 230400            # bench.py's block: 19200 fm samples at the 12-fold decimation
BENCH_HALF = 9600           # prepass_half of a handle of max_block 230400 (work_nj 19216)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("plan") / "call_plan_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "call_plan_check.cpp")])

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [json.loads(line) for line in out]
    return run


def call(n, decim=12, any_rds=0, prepass=0, pllc=0, am=0, call_pieces=-1, channels=4096, ola=0, conv2=0, arrays=1, half=BENCH_HALF):
    return "call %d %d %d %d %d %d %d %d %d %d %d %d" % (n, decim, any_rds, prepass, pllc, am, call_pieces, channels, ola, conv2, arrays, half)


PLL = dict(prepass=1, pllc=1)
AM = dict(prepass=1, pllc=1, am=1)
SQUELCH = dict(prepass=1)


def test_pre_pass_schedules_at_the_bench_block(plan):
    """The pieces of a pre-pass batch's call of 19200 fm samples, in fm samples: the PLL decoder's 4608 with a short last one, the AM decoder's 3840,
    the squelches' equal pieces with the short rest merged, and FMX_P_CALL_PIECES = 3000 (rounded up to 3008, equal pieces)."""
    cases = [(PLL, -1, [4608, 4608, 4608, 3840, 1536]),
             (AM, -1, [3840] * 4 + [2304, 1536]),
             (SQUELCH, -1, [4608, 4608, 4608, 5376]),
             (PLL, 3000, [3008] * 5 + [4160]),
             (SQUELCH, 3000, [3008] * 5 + [4160])]
    got = plan([call(BENCH_N, call_pieces=cp, **kw) for kw, cp, _ in cases])
    for (kw, cp, want), g in zip(cases, got):
        assert g["kind"] == "overlapped", (kw, cp, g)
        assert [l // 12 for l in g["lens"]] == want, (kw, cp, g)
        assert all(l % 12 == 0 for l in g["lens"])


def test_calls_made_whole(plan):
    """A call is made whole without a pre-pass, with FMX_P_CALL_PIECES = 0, on the block machines, behind the second converter, before the pre-pass
    arrays exist, below 1024 channels (automatic), or when it is too short for two pieces."""
    qs = [call(BENCH_N), call(BENCH_N, call_pieces=0, **PLL), call(BENCH_N, ola=1, **PLL), call(BENCH_N, conv2=1, **PLL),
          call(BENCH_N, arrays=0, **PLL), call(BENCH_N, channels=512, **PLL), call(2 * 3072 * 12 - 1, **PLL), call(2 * 4608 * 12 - 1, **SQUELCH)]
    for q, g in zip(qs, plan(qs)):
        assert g == {"kind": "whole", "lens": [int(q.split()[1])]}, (q, g)
    # (an explicit piece length also below 1024 channels)
    g = plan([call(BENCH_N, channels=128, call_pieces=4608, **PLL)])[0]
    assert g["kind"] == "overlapped" and [l // 12 for l in g["lens"]] == [4608, 4608, 4608, 5376], g


def test_rds_pieces(plan):
    """While a channel decodes RDS, a call longer than RDS_BLK - 1 fm samples is made in pieces of that many, one after the other."""
    piece = (RDS_BLK - 1) * 12
    got = plan([call(piece, any_rds=1, **PLL), call(piece + 1, any_rds=1), call(2 * piece + 7, any_rds=1, decim=12)])
    assert got[0] == {"kind": "whole", "lens": [piece]}
    assert got[1] == {"kind": "rds", "lens": [piece, 1]}
    assert got[2] == {"kind": "rds", "lens": [piece, piece, 7]}


@pytest.mark.parametrize("decim,max_block", [(12, 230400), (12, 1000000), (6, 460800), (1, 230400)])
def test_plan_invariants(plan, decim, max_block):
    """Over a sweep of n: the pieces sum to n and are not empty, an overlapping call's pieces fit one half of the pre-pass arrays, an RDS piece covers at
    most RDS_BLK fm samples whatever its phase."""
    half = (((max_block // decim + 2 + 1 + 15) // 16) * 16 // 2) & ~15
    ns = sorted(set(list(range(1, 4000, 7)) + list(range(4000, max_block + 1, 997)) + [max_block]))
    kinds = [dict(), PLL, AM, SQUELCH, dict(any_rds=1), dict(any_rds=1, **PLL), dict(call_pieces=3000, channels=256, **SQUELCH)]
    queries = [call(n, decim=decim, half=half, **kw) for kw in kinds for n in ns]
    seen = set()
    for q, g in zip(queries, plan(queries)):
        n = int(q.split()[1])
        lens = g["lens"]
        seen.add(g["kind"])
        assert sum(lens) == n and all(l > 0 for l in lens), (q, g)
        if g["kind"] == "whole":
            assert lens == [n]
        elif g["kind"] == "overlapped":
            assert len(lens) >= 2 and all(l // decim + 2 <= half for l in lens), (q, g)
        else:
            assert g["kind"] == "rds" and all((l + decim - 1) // decim <= RDS_BLK for l in lens), (q, g)
    assert {"whole", "overlapped"} <= seen
    if max_block // decim > RDS_BLK:
        assert "rds" in seen


def test_two_channel_groups(plan):
    """Stages B and C of a plain batch on 256 CUs: the second group is what is left behind two thirds of the rounds of 768 workgroups, in whole rounds
    (4096 -> 2304 + 1792, 3840 -> 2304 + 1536, 3000 -> 2304 + 696, 2048 -> 1536 + 512, 1536 -> 768 + 768, 1024 -> 768 + 256); one round or less,
    or a second group below 128 channels: one group."""
    want = {4096: 1792, 3840: 1536, 3000: 696, 2048: 512, 1536: 768, 1024: 256, 768: 0, 512: 0, 800: 0, 895: 0, 896: 128}
    got = plan(["second %d 256" % c for c in want])
    assert {c: g["second"] for c, g in zip(want, got)} == want


def test_stage_b_form(plan):
    """Stage B with the rows written: one kernel up to 768 channels, two at 1024 / 2048 / 4096 on 256 CUs; with no rows written: one kernel;
    FMX_P_STAGEB_FORM 1 / 2 forces one / two."""
    chans = [64, 256, 512, 768, 1024, 2048, 4096]
    got = plan(["stageb %d 256 1 0" % c for c in chans] + ["stageb %d 256 0 0" % c for c in chans]
               + ["stageb %d 256 %d 1" % (c, r) for c in chans for r in (0, 1)] + ["stageb %d 256 %d 2" % (c, r) for c in chans for r in (0, 1)])
    two = [g["two"] for g in got]
    k = len(chans)
    assert two[:k] == [0, 0, 0, 0, 1, 1, 1]
    assert two[k:2 * k] == [0] * k
    assert two[2 * k:4 * k] == [0] * (2 * k)
    assert two[4 * k:] == [1] * (2 * k)


def test_stage_a_split_in_time(plan):
    """Stage A's parts (FMX_P_FRONT_PARTS = 0) at 0.1 s blocks on 256 CUs: one channel 25 parts, 256 channels 2, from 512 channels on 1;
    FMX_P_FRONT_PARTS = 1 and handles with twins: 1; a forced count is capped at two tiles per part."""
    n = BENCH_N
    got = plan(["front 0 %d 0 1 1 256" % n, "front 0 %d 0 1 256 256" % n, "front 0 %d 0 1 512 256" % n, "front 0 %d 1 1 1 256" % n,
                "front 0 %d 0 2 1 256" % n, "front 0 %d 32 1 4096 256" % n, "front 0 4000 32 1 1 256", "front 5 %d 0 1 1 256" % n])
    assert got[0] == {"parts": 25, "part_tiles": 6}
    assert got[1] == {"parts": 2, "part_tiles": 75}
    assert got[2]["parts"] == 1 and got[3]["parts"] == 1 and got[4]["parts"] == 1
    assert got[5] == {"parts": 30, "part_tiles": 5}
    assert got[6]["parts"] == 1                     # (3 tiles: not two per part)
    tile = plan(["const"])[0]["FRONT_TILE"]
    for g, r0 in ((got[0], 0), (got[7], 5)):
        nt = (r0 + n - 1) // tile + 1
        assert g["parts"] * g["part_tiles"] >= nt > (g["parts"] - 1) * g["part_tiles"]
