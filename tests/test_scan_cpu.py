"""CPU check of scan mode's arithmetic (sdr-j-fm_amd/csrc/fmx_scan.h): the header's own stage functions, compiled for the host and driven lane
by lane (tests/scan_check.cpp), against a float64 DFT, the reference's own Fft_transform (oracle/_ref, when built) and the reference's float
getSignal / getNoise / get_db (fm-processor.cpp:886-904, fm-constants.h:144)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
SIG = [5 + i for i in range(20)] + [N - 1 - (5 + i) for i in range(20)]            # getSignal's order of summation
NOI = [N // 2 - 1 - (5 + i) for i in range(20)] + [N // 2 + 1 + (5 + i) for i in range(20)]
BINS = np.array(SIG + NOI)


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("scan")
    exe = str(d / "scan_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "scan_check.cpp")])

    def run(blocks):
        blocks = np.ascontiguousarray(blocks, np.complex64).reshape(-1, N)
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        blocks.tofile(fi)
        subprocess.check_call([exe, fi, fo])
        raw = np.fromfile(fo, np.float32).reshape(blocks.shape[0], 2 * N + 2)
        X = raw[:, :2 * N].view(np.complex64)
        return X, raw[:, 2 * N:]
    return run


def ref_db(X):
    """the reference's getSignal / getNoise / get_db in float32, summed in its order"""
    out = []
    for bins in (SIG, NOI):
        s = np.float32(0)
        for k in bins:
            s = np.float32(s + np.float32(abs(np.complex64(X[k]))))
        m = np.float32(s / np.float32(40))
        out.append(np.float32(np.float32(20) * np.log10(np.float32((m + np.float32(1)) / np.float32(256)))))
    return out


def random_blocks(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, N)) + 1j * rng.standard_normal((n, N))).astype(np.complex64) * np.float32(0.3)


def fm_blocks(n, seed):
    """FM at an offset, with a tone, plus a little noise: the signal bins dominate in some blocks, the noise bins in none"""
    rng = np.random.default_rng(seed)
    t = np.arange(n * N) / 192000.0
    out = []
    for off in (0.0, 2500.0, -3000.0, 45000.0):
        ph = 2 * np.pi * off * t + 75000.0 / 1000.0 * np.sin(2 * np.pi * 1000.0 * t)
        x = np.exp(1j * ph) * 0.5 + 0.01 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
        out.append(x.astype(np.complex64).reshape(n, N))
    return np.concatenate(out)


@pytest.mark.parametrize("kind", ["random", "fm"])
def test_spectrum_against_float64_dft(scan, kind):
    blocks = random_blocks(16, 7) if kind == "random" else fm_blocks(4, 11)
    X, _ = scan(blocks)
    ref = np.fft.fft(blocks.astype(np.complex128), axis=1)
    for b in range(blocks.shape[0]):
        scale = np.sqrt(np.sum(np.abs(blocks[b].astype(np.complex128)) ** 2))    # |X| of a 1024-point f32 transform: errors of a few 1e-7 of this
        err = np.abs(X[b, BINS].astype(np.complex128) - ref[b, BINS])
        assert np.all(np.isfinite(X[b, BINS]))
        assert err.max() <= 2e-6 * scale, (b, err.max(), scale)


@pytest.mark.parametrize("kind", ["random", "fm"])
def test_db_values_against_the_references_float_arithmetic(scan, kind):
    blocks = random_blocks(16, 3) if kind == "random" else fm_blocks(4, 5)
    X, db = scan(blocks)
    ref = np.fft.fft(blocks.astype(np.complex128), axis=1).astype(np.complex64)
    for b in range(blocks.shape[0]):
        s, n = ref_db(ref[b])
        assert abs(db[b, 0] - s) <= 1e-3 and abs(db[b, 1] - n) <= 1e-3, (b, db[b], s, n)


def test_against_the_references_fft(scan):
    import oracle_lib as ol
    R = ol.ref()
    if R is None:
        pytest.skip("oracle/_ref (the reference's own classes) not built")
    blocks = np.concatenate([random_blocks(8, 21), fm_blocks(2, 23)])
    X, db = scan(blocks)
    for b in range(blocks.shape[0]):
        v = np.ascontiguousarray(blocks[b]).view(np.float32).copy()
        assert R.ref_fft(ol.fptr(v), N, 0) == 1                       # Fft_transform (scanBuffer, 1024, false)
        Xr = v.view(np.complex64)
        scale = np.sqrt(np.sum(np.abs(blocks[b].astype(np.complex128)) ** 2))
        assert np.abs(X[b, BINS] - Xr[BINS]).max() <= 2e-6 * scale, b
        s, n = ref_db(Xr)
        assert abs(db[b, 0] - s) <= 1e-3 and abs(db[b, 1] - n) <= 1e-3, (b, db[b], s, n)
