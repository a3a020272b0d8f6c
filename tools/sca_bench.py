"""What the sub-carrier decoder costs at the size it is for: 4096 channels, each on a stream of its own, x 0.1 s of signal per call (bench.py's block and
settings), timed with the decoder off, with the modulation meter alone on one channel (the price of the rows: a batch with one decoding channel writes
them for every channel and is no plain batch), with the decoder on one channel, and with it on all channels at 67 kHz.  The method is
tools/mpx_meter_bench.py's: device buffers, a stream of the tool's own, a warm-up, then the mean over the timed calls; the modes alternate, --rounds
times, in one job.  Prints one JSON line per round.

    python tools/sca_bench.py [--channels 4096] [--streams 4096] [--calls 20] [--warmup 5] [--rounds 2] [--modes off,mod_one,one,all] [--tree DIR]

second_group_* is fmx_last_second_group as each mode's handle reports it.  --tree DIR takes the package and its library from another checkout:
--modes off --tree <the parent commit's build> times the same handle on the code without the decoder, in the same job."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METER_MODES = ("one", "all")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="off,mod_one,one,all")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    pkg = importlib.import_module("sdr-j-fm_amd")
    m = pkg.fmx
    C, S, n = args.channels, args.streams, 230400
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    iq = torch.empty((S, n, 2), dtype=torch.float32, device=dev)
    for s0 in range(0, S, 256):                                          # (in slabs: the generator's scratch stays small)
        iq[s0:s0 + 256] = torch.randn((min(256, S - s0), n, 2), generator=g, device=dev) * 0.1
    frames_cap = n // 48 + 96
    pcm = torch.zeros((C, frames_cap, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    for _ in range(args.rounds):
        out = {"tree": "this" if os.path.abspath(args.tree) == ROOT else "other", "channels": C, "streams": S, "samples_per_call": n,
               "signal_seconds_per_call": 0.1, "calls": args.calls}
        for mode in args.modes.split(","):
            f = pkg.Fmx(C, streams=S, stream_of_channel=[c % S for c in range(C)], device=0, max_block=n)
            for pid, v in ((m.P_BANDWIDTH, 165000), (m.P_LF_CUTOFF, 15000), (m.P_DEEMPHASIS, 50), (m.P_VOLUME_DB, -6.0)):
                f.set_param(pid, v)
            if mode == "mod_one":
                f.mod_meter(True, C // 2)
            elif mode in METER_MODES:
                f.sca_enable(67000, C // 2 if mode == "one" else -1)

            def call():
                f.process_device(iq.data_ptr(), n, n, pcm.data_ptr(), frames_cap, hip_stream=stream.cuda_stream)
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            torch.cuda.synchronize()
            out["ms_per_call_decoder_" + mode] = round((time.perf_counter() - t0) * 1e3 / args.calls, 4)
            out["second_group_decoder_" + mode] = f.last_second_group()
            if mode in METER_MODES:
                got = f.sca_read(C // 2, 1, capacity=8, level=False) if mode == "one" else f.sca_read(0, C, capacity=8, level=False)
                out["blocks_read_decoder_" + mode] = int(sum(len(r[1]) for r in got))
            f.close()
        if "ms_per_call_decoder_off" in out:
            for mode in ("mod_one",) + METER_MODES:
                if "ms_per_call_decoder_" + mode in out:
                    out["added_ms_per_call_decoder_" + mode] = round(out["ms_per_call_decoder_" + mode] - out["ms_per_call_decoder_off"], 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
