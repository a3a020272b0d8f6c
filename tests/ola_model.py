"""Float64 models of the reference's two overlap-add filters AS BLOCK MACHINES -- fftFilter (fft-filters.cpp:33-163), the input filter
(2 * 32768 points, 251 taps) and fmAudioFilter (2 * 4096 points, 756 taps) -- across setBandwidth / setlfcutoff in mid-stream, for
sample-by-sample comparisons of FMX_TAP_FM_IQ and FMX_TAP_PRE_RESAMPLER on block-machine handles: numpy and the oracle library's filter
designs only.  A helper module (not a conftest): tests/test_ola_model_cpu.py checks the models against the oracle, re-measures the
constants below and runs the seeded defects; tests/test_gpu_block_machines_per_sample.py holds fmx_ola.hip, fmx_promote.hip and
promote () / demote () to them.

The models know nothing of the library: no step tables, no fused or split path, no promotion.  A machine is four arrays and a counter:
  Pass ()       return C [inp], store the sample at A [inp], and when inp reaches L = fft_size - degree run the block transform
  transform     C [k] = sum_i h [i] A [k - i] (+ Overloop [k] for k < degree); the new Overloop is the tail L ... L + degree - 1 of that
                convolution, whose last entry is zero (L + degree - 1 terms)
  setLowPass    a new kernel and inp = 0; A, C and Overloop stay: the last block is played again, the block in progress is dropped, the
                old tail is added to the first block of the new kernel
  "Off"         the samples pass undelayed, the machine keeps its state
Settings are taken over at call boundaries (fm-processor.cpp:396-408).

Numbering: the input machine counts input samples, the audio machine fm samples; a call that begins at input sample p begins at fm
sample p // 12 (the decimators' counters run on across calls).
"""
import ctypes as C

import numpy as np

import f64_models as fm
import stage_a_model as sa
import stage_b_model as sb

IN_FFT, IN_TAPS = 2 * 32768, 251          # inputFilter fm-processor.cpp:77
AU_FFT, AU_TAPS = 2 * 4096, 756           # fmAudioFilter :76
IN_L, AU_L = IN_FFT - IN_TAPS, AU_FFT - AU_TAPS          # 65285 input samples, 7436 fm samples
RATE, FM_RATE, DECIM = 2304000, 192000, 12
PROMO_REACH = 2 * AU_L                    # fm samples behind a promotion whose audio output depends on reconstructed input

DEFECTS = ("clear_overloop", "no_replay", "position_off_by_one", "drop_overloop_entry", "drop_overloop_head", "off_clears_c")


# ------------------------------------------------------------------------------------------------ the machine
class BlockMachine:
    """fftFilter restated.  run (x) is Pass () over the samples x ([n] complex or real) in slices that end at the block boundary.
    marks: (samples seen, on, block since the last restart, inp) at the start and at every setter -- what the locator reads.
    defect: one of DEFECTS, a seed for the detector (tests/test_ola_model_cpu.py)."""

    def __init__(self, fft_size, degree, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.N, self.D, self.L = int(fft_size), int(degree), int(fft_size) - int(degree)
        self.A = np.zeros(self.L, np.complex128)
        self.C = np.zeros(self.L, np.complex128)
        self.over = np.zeros(self.D, np.complex128)
        self.h = np.zeros(self.D)
        self.inp, self.on, self.block, self.seen = 0, False, 0, 0
        self.defect = defect
        self.marks = [(0, False, 0, 0)]

    def _mark(self):
        self.marks.append((self.seen, self.on, self.block, self.inp))

    def set_lowpass(self, taps):
        taps = np.asarray(taps, np.float64)
        assert taps.shape == (self.D,)
        self.h = taps.copy()
        self.on = True
        if self.defect != "no_replay":
            self.inp, self.block = (1 if self.defect == "position_off_by_one" else 0), 0
        if self.defect == "clear_overloop":
            self.over[:] = 0.0
        self._mark()

    def off(self):
        self.on = False
        if self.defect == "off_clears_c":
            self.C[:] = 0.0
        self._mark()

    def _transform(self):
        y = fm.fftconv(self.A, self.h)                       # [L + D - 1]
        self.C = y[:self.L].copy()
        self.C[:self.D] += self.over
        self.over[:self.D - 1] = y[self.L:]
        self.over[self.D - 1] = 0.0
        if self.defect == "drop_overloop_entry":
            self.over[self.D - 2] = 0.0
        if self.defect == "drop_overloop_head":
            self.over[0] = 0.0
        self.block += 1

    def run(self, x):
        x = np.asarray(x, np.complex128)
        n = x.shape[0]
        if not self.on:
            self.seen += n
            return x.copy()
        out = np.empty(n, np.complex128)
        i = 0
        while i < n:
            k = min(n - i, self.L - self.inp)
            out[i:i + k] = self.C[self.inp:self.inp + k]
            self.A[self.inp:self.inp + k] = x[i:i + k]
            self.inp += k
            i += k
            if self.inp >= self.L:
                self.inp = 0
                self._transform()
        self.seen += n
        return out


def run_events(machine, x, events, kernel_of):
    """The stream x through `machine`; events: [(position, value | 0)] in the machine's own sample numbering, ascending, position 0 = the
    setting in force at the stream's start; kernel_of (value) -> taps.  -> the machine's output [n]."""
    n = x.shape[0]
    ev = sorted(((int(p), int(v)) for p, v in events), key=lambda e: e[0])          # (setters at one position keep their order)
    assert ev and ev[0][0] == 0 and all(0 <= p <= n for p, _ in ev)
    out = np.empty(n, np.complex128)
    bounds = [p for p, _ in ev[1:]] + [n]
    for (p, v), q in zip(ev, bounds):
        if v > 0:
            machine.set_lowpass(kernel_of(v))
        else:
            machine.off()
        out[p:q] = machine.run(x[p:q])
    return out


def locate(marks, index, length):
    """(on, block since the last restart, position in the block) of sample `index` of a machine's stream from its marks."""
    m = [k for k in marks if k[0] <= index][-1]
    if not m[1]:
        return False, 0, int(index - m[0])
    q = m[3] + int(index - m[0])
    return True, m[2] + q // length, q % length


# ------------------------------------------------------------------------------------------------ designs
_kernels = {}


def input_kernel(L, bw):
    """The reference's 251 input-filter taps of a bandwidth (f32 from the oracle's design, as float64)."""
    key = ("in", int(bw))
    if key not in _kernels:
        _kernels[key] = sa.Design(L, RATE, int(bw)).h_in
    return _kernels[key]


def with_echo(h, echo):
    """The kernel h with `echo` added to its LAST tap.  The windowed designs end in taps of 2.2e-8 (input filter) and 1.5e-9 (audio filter), so what
    the last non-zero tail entry, Overloop [degree - 2] = h [degree - 1] A [L - 1], carries is below the resolution of f32 samples; a seeded defect in
    that entry is run on a kernel whose last tap has weight (tests/test_ola_model_cpu.py).  echo = 0: h itself."""
    if not echo:
        return h
    g = np.array(h, np.float64)
    g[-1] += float(echo)
    return g


def audio_kernel(L, cutoff):
    key = ("au", int(cutoff))
    if key not in _kernels:
        h = np.zeros(AU_TAPS, np.float32)
        L.fmo_lowpass_kernel(AU_TAPS, int(cutoff), FM_RATE, h.ctypes.data_as(C.POINTER(C.c_float)))
        _kernels[key] = h.astype(np.float64)
    return _kernels[key]


# ------------------------------------------------------------------------------------------------ call lists and events
def boundaries(calls):
    return np.concatenate([[0], np.cumsum(calls)]).astype(np.int64)


def input_events(calls, first, at_call):
    """[(input-sample position, bandwidth | 0)]: `first` in force from the start, at_call: {call index: value} taken over at that call's
    first sample."""
    b = boundaries(calls)
    return [(0, int(first))] + [(int(b[k]), int(v)) for k, v in sorted(at_call.items())]


def audio_events(calls, first, at_call):
    """[(fm-sample position, cut-off | 0)]: a call that begins at input sample p begins at fm sample p // 12."""
    b = boundaries(calls)
    return [(0, int(first))] + [(int(b[k]) // DECIM, int(v)) for k, v in sorted(at_call.items())]


def late(at_call, by=1):
    """A seed for the detector: every setter taken one call late."""
    return {k + by: v for k, v in at_call.items()}


# ------------------------------------------------------------------------------------------------ the input side
def premix(x, calls=None, lo=0, att=(1.0, 1.0), dc_remove=1):
    """The samples in front of the input filter in the reference's order (fm-processor.cpp:423-466): RF DC removal, balance, oscillator."""
    x = sa.as_complex(x)
    LO, _ = sa.oscillator(x.shape[0], RATE, sa.per_call(lo, calls))
    R = sa.rf_dc(x, RATE, sa.per_call(dc_remove, calls))
    return sa.balance(x - sa.clamp(R[1:]), att) * LO


class InputSide:
    """FMX_TAP_FM_IQ of one channel over a whole stream: premix, the input machine across `events`, fmBand_1, fmBand_2 (stage_a_model's
    filters with the machine in the LTI filter's place).  z [n / 12] complex128; marks: the machine's, in input samples."""

    def __init__(self, L, x, calls, events, lo=0, att=(1.0, 1.0), dc_remove=1, defect=None, v=None, echo=0.0):
        self.D = sa.Design(L, RATE, 165000)               # (the decimators: the same for every bandwidth)
        self.machine = BlockMachine(IN_FFT, IN_TAPS, defect)
        self.v = premix(x, calls, lo, att, dc_remove) if v is None else v
        self.w = run_events(self.machine, self.v, events, lambda bw: with_echo(input_kernel(L, bw), echo))
        self.z = sa.filters(self.v, self.D, filtered=self.w)
        self.marks = self.machine.marks

    def where(self, j):
        """fm sample j's newest input sample, in the machine's terms."""
        return locate(self.marks, DECIM * int(j) + DECIM - 1, IN_L)


# ------------------------------------------------------------------------------------------------ the audio side
class AudioSide:
    """FMX_TAP_PRE_RESAMPLER of a block-machine handle from that handle's own LR_RAW [n, 2] f32: the stereo matrix in the reference's f32
    expressions, the audio machine across `events` (fm samples), the de-emphasis in float64 (fm-processor.cpp:517-549, 589-595).
    y [n, 2] float64.  deemph_first: a seed for the detector, the de-emphasis in front of the filter."""

    def __init__(self, L, lr_raw, events, selector=0, fm_mode=0, panorama=100, deemph_us=50, defect=None, deemph_first=False, x=None, echo=0.0):
        m = sb.matrix_f32(lr_raw, selector, fm_mode, panorama).astype(np.float64) if x is None else np.asarray(x, np.float64)
        alpha = sb.deemph_alpha(deemph_us)
        if deemph_first:
            m = sb.one_pole_f64(m, alpha)
        self.machine = BlockMachine(AU_FFT, AU_TAPS, defect)
        self.x = m
        f = run_events(self.machine, m[:, 0] + 1j * m[:, 1], events, lambda c: with_echo(audio_kernel(L, c), echo))
        self.filtered = np.stack([f.real, f.imag], axis=1)
        self.y = self.filtered if deemph_first else sb.one_pole_f64(self.filtered, alpha)
        self.marks = self.machine.marks

    def where(self, j):
        return locate(self.marks, int(j), AU_L)


def inverted_deemphasis_f32(y32, alpha):
    """promo_inv_deemph_kernel restated in numpy f32: x [n] = (y [n] - y [n - 1]) (1 / a) + y [n - 1], y [-1] = 0; y32 [n, 2] f32."""
    y = np.asarray(y32, np.float32)
    yp = np.concatenate([np.zeros((1, y.shape[1]), np.float32), y[:-1]])
    ra = np.float32(1.0) / np.float32(alpha)
    return ((y - yp) * ra + yp).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the comparison both test modules use
class Report:
    def __init__(self, name, rel, err, index, scale, call, on, block, position, bound):
        self.name, self.rel, self.err, self.index, self.scale, self.call = name, rel, err, index, scale, call
        self.on, self.block, self.position, self.bound = on, block, position, bound

    def __str__(self):
        place = "block %d since the last restart, position %d" % (self.block, self.position) if self.on else "filter off, %d samples behind the switch" % self.position
        return ("[%s] worst sample %.3e of the peak %.4g (%.3e) at fm sample %d: call %d, %s; bound %.3e"
                % (self.name, self.rel, self.scale, self.err, self.index, self.call, place, self.bound))


def judge(name, got, ref, call_starts, where, bound, check=True):
    """Every sample of `got` ([n, 2] f32, or complex) against `ref` ([n] complex128 or [n, 2] float64), per component, relative to the
    reference's peak.  where (fm sample) -> (on, block, position).  Prints the line, asserts (check), -> Report of the worst sample."""
    g = np.asarray(got)
    g = np.stack([g.real, g.imag], axis=1) if np.iscomplexobj(g) else g.astype(np.float64)
    r = np.asarray(ref)
    r = np.stack([r.real, r.imag], axis=1) if np.iscomplexobj(r) else r.astype(np.float64)
    assert g.shape == r.shape and g.shape[0] > 0, (name, g.shape, r.shape)
    peak = float(np.abs(r).max())
    assert peak > 0, name
    e = np.abs(g - r).max(axis=1)
    i = int(np.argmax(e))
    cs = np.asarray(call_starts, np.int64)
    call = max(int(np.searchsorted(cs, i, side="right") - 1), 0)
    on, block, position = where(i)
    rep = Report(name, float(e[i]) / peak, float(e[i]), i, peak, call, on, block, position, float(bound))
    print("\n%s" % rep)
    if check:
        assert rep.rel <= rep.bound, "beyond the bound -- %s" % rep
    return rep


def call_starts_fm(calls):
    return [int(p) // DECIM for p in boundaries(calls)[:-1]]


# ------------------------------------------------------------------------------------------------ which path a call takes
def coverage(calls, first, at_call, length, fm):
    """What the library's host has to decide for every call of a handle, from the models' own block counters (the kernels cannot say which
    path ran).  at_call: per channel {call: value | 0} of one side, `first` in force from the start; length: the machine's L; fm: the audio
    side (a call's samples are the fm samples it completes).  -> per call a set of:
      whole     every running filter takes the call without completing a block (the fused path)
      exact     every running filter's block ends with the call's last sample (fused, the transform behind it)
      crosses   some filter crosses a block boundary inside the call (the split path); several: more than one boundary
      differ    running filters of the handle at different block positions at the call's first sample
      one       a call of one input sample
      empty     a call without a sample for this side at which a setter is taken over"""
    b = boundaries(calls)
    pos = b // DECIM if fm else b
    state = [dict(on=first > 0, inp=0) for _ in at_call]
    out = []
    for k in range(len(calls)):
        n = int(pos[k + 1] - pos[k])
        flags, inps, ends, setter = set(), [], [], False
        for st, ev in zip(state, at_call):
            if k in ev:
                setter = True
                st["on"] = ev[k] > 0
                if ev[k] > 0:
                    st["inp"] = 0
            if st["on"]:
                inps.append(st["inp"])
                ends.append(st["inp"] + n)
                st["inp"] = (st["inp"] + n) % length
        if calls[k] == 1:
            flags.add("one")
        if n == 0 and setter:
            flags.add("empty")
        if ends and n > 0:
            if all(e < length for e in ends):
                flags.add("whole")
            elif all(e == length for e in ends):
                flags.add("exact")
            if any(e > length for e in ends):
                flags.add("crosses")
            if any(e > 2 * length for e in ends):
                flags.add("several")
        if len(set(inps)) > 1:
            flags.add("differ")
        out.append(flags)
    return out


def position_at_setters(calls, first, at_call, length, fm):
    """{call: (running, inp)} of one channel's machine just in front of each of its setters."""
    b = boundaries(calls)
    pos = b // DECIM if fm else b
    on, inp, out = first > 0, 0, {}
    for k in range(len(calls)):
        if k in at_call:
            out[k] = (on, inp)
            on = at_call[k] > 0
            inp = 0 if on else inp
        if on:
            inp = (inp + int(pos[k + 1] - pos[k])) % length
    return out


REQUIRED =("whole", "exact", "crosses", "several", "differ", "one")


# ------------------------------------------------------------------------------------------------ the shapes the CPU and the GPU tests share
RAGGED = sb.RAGGED                      # [50000, 12, 13, 99999, 230400, 1, 100000]: the 230400-sample call is 29 tiles of pre_kernel's look-back
# The head: the input machine's first block ends with call 0 (65285 = L), the audio machine's with call 1 (65285 + 23947 = 89232 = 12 x
# 7436); call 2 ends at 130569 = 65285 + 65284 (a channel restarted at 65285 stands at inp = L - 1 there) and call 3 at 178452 = 12 x
# 14871, fm sample 7436 + 7435 (an audio machine restarted at 7436 stands at L - 1).
R_CALLS = [65285, 23947, 41337, 47883] + RAGGED * 3          # 1 619 727 input samples, 25 calls
R_STREAM = [0, 1, 0, 1, 0, 1]
R_DC = [(0.0, 0.0), (0.004, -0.003)]
# per channel: settings (stage A's kinds), {call: bandwidth} and {call: cut-off} taken over at that call's first sample
R_KINDS = [dict(), dict(), dict(), dict(), dict(lo=2500, att_l=0.9, att_r=1.1), dict()]
R_BW = [{}, {7: 120000, 10: 120000}, {7: 0, 10: 165000}, {}, {8: 130000}, {1: 130000, 3: 165000}]
R_LF = [{}, {}, {}, {5: 9000, 9: 0, 14: 15000}, {8: 12000}, {2: 12000, 4: 15000}]
R_SINGLE_BW, R_SINGLE_LF = R_BW[1], R_LF[3]                 # the one-channel handle: channel 1's and channel 3's events
BW0, LF0 = 165000, 15000


def r_input_events(c, defect_late=False):
    ev = R_BW[c] if not defect_late else late(R_BW[c])
    return input_events(R_CALLS, BW0, ev)


def r_audio_events(c, defect_late=False):
    ev = R_LF[c] if not defect_late else late(R_LF[c])
    return audio_events(R_CALLS, LF0, ev)


def r_streams(ol, n=None):
    n = sum(R_CALLS) if n is None else n
    return np.stack([ol.synth_iq(n, leftHz=1000.0 + 370.0 * s, rightHz=400.0 + 230.0 * s, dcI=d[0], dcQ=d[1], pilotLevel=0.12) for s, d in enumerate(R_DC)])


# case p: 40 calls of 49152 samples
P_CALLS = [49152] * 40


# ------------------------------------------------------------------------------------------------ the reference's own distance
# Worst sample, relative to the stream's peak, of the oracle's f32 arithmetic against these models on identical inputs; measured by
# tests/test_ola_model_cpu.py, which prints every figure and fails if a record understates what it sees.  The GPU bounds are the records
# doubled (the suite's convention for another summation order: ola_conv_kernel's direct convolution in place of f32 FFTs) and come from
# nothing else.
REF_OLA_IN_FILTER = 8.83e-7     # fmo_fftfilter (65536, 251) against BlockMachine over the schedule of test_oracle_filter_against_the_machine: 11.4 blocks, 6 setters (measured 8.823e-7, peak 0.60)
REF_OLA_AU_FILTER = 5.40e-7     # fmo_fftfilter (8192, 756) likewise (measured 5.399e-7, peak 0.64)
REF_OLA_IN_CHAIN = 9.61e-7      # OracleChain TAP_FM_IQ against InputSide over R_CALLS with the setters of case r, worst of the six channels (7.2e-7 ... 9.600e-7, peaks 2.5 ... 2.7)
REF_OLA_AU_CHAIN = 9.22e-7      # OracleChain TAP_PRE_RS against AudioSide on the oracle's own TAP_LRRAW, likewise (6.6e-7 ... 9.216e-7, peak 0.70): f32 FFTs and the f32 de-emphasis
REF_INV_DEEMPH = 3.57e-7        # the float64 audio machine on the f32-inverted de-emphasis against the same machine on the true stream (measured 3.562e-7; the reconstruction itself 2.1e-7)
OLA_AU_BOUND = 2.0 * max(REF_OLA_AU_FILTER, REF_OLA_AU_CHAIN)
OLA_AU_BOUND_PROMOTED = OLA_AU_BOUND + 2.0 * REF_INV_DEEMPH


OLA_IN_BOUND = max(2.0 * max(REF_OLA_IN_FILTER, REF_OLA_IN_CHAIN), sa.STAGE_A_BOUND_ON)      # stage A keeps one bound where the machines' own figure is not larger
