"""The binding a maintainer adds to the reference tree, compiled for real: the three replacement sources of
sdr-j-fm_amd/host/reference_tree -- fm-processor-fmx.cpp, fm-demodulator-fmx.cpp, rds-decoder-fmx.cpp -- against the REFERENCE'S OWN
headers (includes/fm/fm-processor.h, fm-demodulator.h, includes/rds/rds-decoder.h, devices/device-handler.h, includes/various/ringbuffer.h
and everything they include), plus the moc output of those QObject headers, with the image's Qt 5.9.  Compile only (g++ -c): the GUI,
PortAudio, libsndfile and libsamplerate are not in the image (tests/shim_headers/README.md says what stands in for their headers).
Every member function and signal the reference's fm-processor.h / rds-decoder.h / fm-demodulator.h declare must be defined with the
declared signature -- a mismatch (setDeemphasis (int16_t), setfmRdsSelector (rdsDecoder::ERdsMode), ...) fails here.  CPU only; skipped
where the reference tree or Qt is absent."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
QT = "/opt/conda"
MOC = os.path.join(QT, "bin", "moc")
BIND = os.path.join(ROOT, "sdr-j-fm_amd", "host", "reference_tree")
SHIM = os.path.join(ROOT, "tests", "shim_headers")

needs_ref = pytest.mark.skipif(not (os.path.isdir(os.path.join(REF, "includes")) and os.path.exists(MOC)),
                               reason="needs the reference tree and the image's Qt (moc, QtCore headers)")

INCS = ["-I" + SHIM, "-I" + BIND, "-I" + os.path.join(ROOT, "include")] + \
       ["-I" + os.path.join(REF, d) for d in ("includes", "includes/fm", "includes/rds", "includes/various", "devices")] + \
       ["-I" + os.path.join(QT, "include", "qt")] + ["-I" + os.path.join(QT, "include", "qt", m) for m in ("QtCore", "QtGui", "QtWidgets")]
CXX = ["g++", "-std=c++17", "-O1", "-fPIC", "-w", "-c"]


def compile_obj(src, out):
    subprocess.check_call(CXX + INCS + [src, "-o", out])
    return out


def defined_symbols(obj):
    txt = subprocess.check_output(["nm", "-C", "--defined-only", obj]).decode()
    return txt


@needs_ref
def test_binding_compiles_against_the_reference_headers(tmp_path):
    objs = {}
    for name in ("fm-processor-fmx.cpp", "fm-demodulator-fmx.cpp", "rds-decoder-fmx.cpp"):
        objs[name] = compile_obj(os.path.join(BIND, name), str(tmp_path / (name + ".o")))
    # the moc output of the reference's own QObject headers compiles next to it (signals = the reference's)
    for hdr in ("includes/fm/fm-processor.h", "includes/rds/rds-decoder.h"):
        m = str(tmp_path / ("moc_" + os.path.basename(hdr).replace(".h", ".cpp")))
        subprocess.check_call([MOC] + [i for i in INCS if not i.startswith("-I" + QT)] + [os.path.join(REF, hdr), "-o", m])
        compile_obj(m, m + ".o")
    # every non-inline member function the reference's class declarations name is defined by the replacement, with that signature
    want = {"fm-processor-fmx.cpp": ("includes/fm/fm-processor.h", "fmProcessor"),
            "fm-demodulator-fmx.cpp": ("includes/fm/fm-demodulator.h", "fm_Demodulator"),
            "rds-decoder-fmx.cpp": ("includes/rds/rds-decoder.h", "rdsDecoder")}
    for src, (hdr, cls) in want.items():
        syms = defined_symbols(objs[src])
        text = open(os.path.join(REF, hdr)).read()
        body = text[text.index("class " + cls if cls != "fm_Demodulator" else "class\tfm_Demodulator"):]
        body = body[:body.index("signals:")] if "signals:" in body else body[:body.index("};")]
        names = set(re.findall(r"\b([A-Za-z_][A-Za-z_0-9]*)\s*\(", re.sub(r"//.*", "", body)))
        names -= {cls, "DSPCOMPLEX", "DelayLine", "defined", "std", "complex", "float", "RingBuffer", "if", "sizeof", "int32_t"}
        for n in sorted(names):
            if not re.search(r"\b%s::%s\(" % (cls, n), syms):
                # (an enum, a member with an initialiser or an inline function is not a function to define)
                assert re.search(r"\b%s\s*\([^;{]*\)\s*(const)?\s*;" % n, body) is None, "%s::%s is declared by %s and not defined by %s" % (cls, n, hdr, src)
        assert re.search(r"\b%s::%s\(" % (cls, cls), syms) and re.search(r"\b%s::~%s\(" % (cls, cls), syms)
    s = defined_symbols(objs["fm-processor-fmx.cpp"])
    assert "fmProcessor::setDeemphasis(short)" in s and "fmProcessor::setfmRdsSelector(rdsDecoder::ERdsMode)" in s
    assert "fmProcessor::startDumping(sf_private_tag*)" in s and "fmProcessor::run()" in s


# ---- link and run (VERDICT r3 next #9c) --------------------------------------------------------------------------------------------------
# The recipe is oracle/build_ref_tree_demo.py (it compiles reference sources in place, so its output belongs in oracle/_ref/, which travels
# to the GPU box); the GPU test runs the executable built here.
import importlib.util  # noqa: E402

_spec = importlib.util.spec_from_file_location("build_ref_tree_demo", os.path.join(ROOT, "oracle", "build_ref_tree_demo.py"))
DEMO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(DEMO)
# (the libfmx.so under test is this tree's build, named to the loader here: the executable in oracle/_ref/ may have been linked in another
# checkout, and its own search path then points there)
RUN_ENV = dict(os.environ, LD_LIBRARY_PATH=DEMO.LIBDIR + ":" + os.path.join(QT, "lib"), LD_PRELOAD=":".join(filter(None, (os.environ.get("LD_PRELOAD"), "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"))), QT_QPA_PLATFORM="offscreen")


def test_binding_links_with_the_reference_rds_classes():
    if not DEMO.available():
        pytest.skip("needs the reference tree, Qt and libfmx.so")
    exe = DEMO.build()
    syms = subprocess.check_output(["nm", "-C", "--defined-only", exe]).decode()
    # the reference's own classes are in the executable next to the binding
    for s in ("rdsBlockSynchronizer::pushBit", "rdsGroupDecoder::decode", "RDSGroup::", "fmProcessor::run()", "rdsDecoder::processBit"):
        assert s in syms, s
    r = subprocess.run([exe], env=RUN_ENV, capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_binding_runs_the_reference_rds_classes_on_gpu_bits(tmp_path, ol, fmx_amd):
    """The run: a stereo station with an RDS programme (PI D3A1, PS "FMX-AMD ", a radio text) as a raw IQ file through the reference-header
    fmProcessor of fm-processor-fmx.cpp; libfmx demodulates and slices, the REFERENCE'S OWN rdsBlockSynchronizer / rdsGroupDecoder decode the
    bits and their Qt signals reach the GUI stand-in; the PCM that reached the audioSink equals the oracle's."""
    import numpy as np
    exe = DEMO.OUT
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_tree_demo was not built (python oracle/build_ref_tree_demo.py where the reference tree is)")
    seconds = 2.6
    n = int(seconds * 2304000) // 16384 * 16384
    iq = ol.synth_iq(n, rds=1, rdsLevel=0.05, rds_payload=ol.rds_programme_bits(pi=0xD3A1, ps="FMX-AMD ", text="REFERENCE CLASSES ON GPU BITS"))
    (tmp_path / "iq.f32").write_bytes(np.ascontiguousarray(iq, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "iq.f32"), str(seconds), str(tmp_path / "pcm.f32")], env=RUN_ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = r.stdout.strip().splitlines()[-2].split()
    kv = dict(zip(line[0::2], line[1::2]))
    txt = dict(f.split("=", 1) for f in r.stdout.strip().splitlines()[-1].split("|"))
    print("\n[reference-tree binding, linked and run]", kv, txt)
    assert kv["pi"] == "D3A1" and int(kv["groups"]) >= 20 and kv["synced"] == "1" and kv["locked"] == "1"
    assert txt["label"].strip() == "FMX-AMD" and "REFERENCE CLASSES ON GPU BITS" in txt["text"]
    pcm = np.frombuffer((tmp_path / "pcm.f32").read_bytes(), np.float32).reshape(-1, 2)
    po = ol.OracleChain(inputFilterBw=165000, rdsMode=2).process(iq)
    m = min(len(pcm), len(po))
    assert m >= len(po) - 400 and float(np.sqrt(np.mean((pcm[:m].astype(np.float64) - po[:m]) ** 2))) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("rate,bw", [(2048000, "165kHz"), (192000, "Off")])
def test_binding_runs_at_the_rates_decimated_by_6_and_by_1(tmp_path, ol, fmx_amd, rate, bw):
    """the reference-tree fmProcessor at a device rate the reference decimates by 6 (rtl-sdr's 2.048 MS/s: 683 PCM frames
    per 16384-sample block) and at one it does not decimate (192 kS/s: 4096 frames per block) -- its PCM buffer is sized by fmx_frames_for,
    every block reaches the audioSink, and the PCM equals the oracle's chain built for that rate."""
    import numpy as np
    exe = DEMO.OUT
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_tree_demo was not built (python oracle/build_ref_tree_demo.py where the reference tree is)")
    decim = 1 if rate // 192000 <= 1 else 6 * ((rate // 6) // 192000)
    n = 16384 * (60 if decim > 1 else 12)
    iq = ol.synth_iq(n)                              # (generator time base 2.304 MS/s; the receivers are told `rate`)
    (tmp_path / "iq.f32").write_bytes(np.ascontiguousarray(iq, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "iq.f32"), "0", str(tmp_path / "pcm.f32"), str(rate), bw], env=RUN_ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "pcm_stride" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    pcm = np.frombuffer((tmp_path / "pcm.f32").read_bytes(), np.float32).reshape(-1, 2)
    po = ol.OracleChain(inputRate=rate, inputFilterBw=0 if bw == "Off" else 165000, rdsMode=2).process(iq)
    m = min(len(pcm), len(po))
    print("\n[reference-tree binding at %d S/s] frames %d (oracle %d)" % (rate, len(pcm), len(po)))
    assert m >= len(po) - 16384 // decim // 4 - 8 and m > 0.9 * (n // decim // 4)
    assert float(np.sqrt(np.mean((pcm[:m].astype(np.float64) - po[:m]) ** 2))) <= 1e-5
