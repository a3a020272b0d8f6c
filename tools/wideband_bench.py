"""Stage W (wide-band ingest) at the size it is for: 8 streams at K = 8 (18.432 MS/s) x 96 stations each x 0.1 s per call, alone and chained
into a 768-channel handle (bench.py's config4 settings) on one stream with no copy in between.  Times the calls after a warm-up and prints
one JSON line: ms per call of each form, the real-time factor of the chained form (0.1 s of signal per call), the HBM bytes the stage reads
per wide sample -- ALGORITHMIC, not counted: every sample once per stream plus the 16 history columns a tile of 256 re-reads; the rotator
table's gathers and the tap fetches that miss the caches are not in it -- and the fraction of the HBM copy bound the stage alone reaches
(bytes it must move: every wide sample once in, every narrow sample once out, over 8 TB/s).

    python tools/wideband_bench.py [--streams 8] [--factor 8] [--stations 96] [--calls 20] [--warmup 5] [--format f32|u8|s8|s16] [--survey B] [--rate HZ]

--survey B (blocks of 4096 wide samples per record, 1 .. 4096): the same stage-W calls timed once more with the band survey on
(fmx_wideband_survey_enable), beside the time with it off from the same run; the line then also holds the survey's added ms per call and the
scratch bytes it writes and reads again per call (4 B each per wide sample: ALGORITHMIC, as above).

--rate HZ: a rate object (fmx_wideband_create_rate, fmx_wide_rate.hip) for a stream of HZ S/s in place of the factor: 0.1 s of signal per call
as before, HZ / 10 wide samples.  The line then holds the ratio L / M and the time per (wide sample x station) in ps, which the factor form
reports too, so that the two forms can be set side by side.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
TILE, HIST_COLS = 256, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--factor", type=int, default=8)
    ap.add_argument("--stations", type=int, default=96)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--format", default="f32", choices=["f32", "u8", "s8", "s16"])
    ap.add_argument("--survey", type=int, default=0, metavar="B")
    ap.add_argument("--rate", type=int, default=0, metavar="HZ")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sdr-j-fm_amd")
    m = pkg.fmx
    K, S, per = args.factor, args.streams, args.stations
    C = S * per
    n_narrow = 230400                                 # 0.1 s at 2 304 000 S/s: bench.py's block
    n_wide = n_narrow * K
    taps_per_output = 16 * K + 1
    if args.rate:
        h, L, M = m.wideband_rate_taps(args.rate)     # (refused rates end here with the library's text)
        K, n_wide = 0, args.rate // 10
        n_narrow = n_wide * L // M + 1                # a call produces floor (n L / M) outputs or one more
        taps_per_output = -(-len(h) // L)
    fmt, dt, bps = {"f32": (m.IQ_F32, torch.float32, 8), "u8": (m.IQ_U8, torch.uint8, 2), "s8": (m.IQ_S8, torch.int8, 2),
                    "s16": (m.IQ_S16, torch.int16, 4)}[args.format]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    if dt == torch.float32:
        wide = (torch.randn((S, n_wide, 2), generator=g, device=dev) * 0.1).contiguous()
    else:
        lo, hi = {torch.uint8: (0, 256), torch.int8: (-128, 128), torch.int16: (-2048, 2048)}[dt]
        wide = torch.randint(lo, hi, (S, n_wide, 2), generator=g, device=dev, dtype=dt).contiguous()
    narrow = torch.zeros((C, n_narrow, 2), dtype=torch.float32, device=dev)
    frames_cap = n_narrow // 48 + 96
    pcm = torch.zeros((C, frames_cap, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    lim = (args.rate // 2 if args.rate else K * 1152000) - 150000
    sof = [c // per for c in range(C)]
    offs = [int(-lim + (2 * lim) * (c % per) / max(per - 1, 1)) for c in range(C)]      # the stations spread over the stream's band
    out = {"streams": S, "factor": K, "rate_hz": args.rate or K * 2304000, "stations_per_stream": per, "outputs": C, "format": args.format, "wide_samples_per_call": n_wide,
           "signal_seconds_per_call": 0.1, "calls": args.calls}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    w = pkg.Wideband(K, sof, offs, streams=S, max_block=n_wide, rate_hz=args.rate or None)
    if args.rate:
        out["L"], out["M"] = L, M
    last = {"n": n_narrow}

    def stage_w():
        last["n"] = w.process_device(wide.data_ptr(), n_wide, n_wide, narrow.data_ptr(), n_narrow, fmt=fmt, hip_stream=stream.cuda_stream)

    out["ms_per_call_stage_w"] = round(timed(stage_w), 4)
    out["ps_per_wide_sample_and_station"] = round(out["ms_per_call_stage_w"] * 1e9 / (n_wide * C), 3)
    if args.survey > 0:
        w.survey(args.survey)
        out["survey_blocks_per_record"] = args.survey
        out["ms_per_call_stage_w_survey_on"] = round(timed(stage_w), 4)
        out["survey_added_ms_per_call"] = round(out["ms_per_call_stage_w_survey_on"] - out["ms_per_call_stage_w"], 4)
        out["survey_records_read_stream0"] = int(len(w.survey_read(0)[0]))
        out["survey_scratch_bytes_written_and_read_per_call"] = 2 * 4 * (n_wide // 4096 * 4096) * S
        w.survey(0)
    f = pkg.Fmx(C, device=0, max_block=n_narrow)
    for pid, v in ((m.P_BANDWIDTH, 165000), (m.P_LF_CUTOFF, 15000), (m.P_DEEMPHASIS, 50), (m.P_VOLUME_DB, -6.0)):
        f.set_param(pid, v)

    def handle():
        f.process_device(narrow.data_ptr(), n_narrow, last["n"], pcm.data_ptr(), frames_cap, hip_stream=stream.cuda_stream)

    def chained():
        stage_w()
        handle()

    out["ms_per_call_handle_alone"] = round(timed(handle), 4)
    out["ms_per_call_chained"] = round(timed(chained), 4)
    out["chained_real_time_factor"] = round(100.0 / out["ms_per_call_chained"], 2)
    out["chained_faster_than_real_time"] = out["ms_per_call_chained"] < 100.0
    # what the stage must read from HBM per wide sample (algorithmic): the sample itself, once, plus the 16 history columns every tile of 256 re-reads
    out["algorithmic_hbm_bytes_read_per_wide_sample"] = round(bps * (1 + (taps_per_output - 1) / (TILE * M / L)), 3) if args.rate else round(bps * (TILE + HIST_COLS) / TILE, 3)
    must_move = S * n_wide * bps + C * n_narrow * 8
    out["stage_w_bytes_moved_per_call"] = must_move
    out["stage_w_fraction_of_hbm_copy_bound"] = round(must_move / HBM_BYTES_PER_S * 1e3 / out["ms_per_call_stage_w"], 4)
    out["stage_w_tflops_f32"] = round(C * last["n"] * taps_per_output * 8 / (out["ms_per_call_stage_w"] * 1e-3) / 1e12, 2)
    w.close()
    f.close()
    print(json.dumps(out))
    assert out["chained_faster_than_real_time"], "the chained form must process 0.1 s of signal in less than 0.1 s"


if __name__ == "__main__":
    main()
