"""What the monitoring feed costs at the size it is for: 4096 channels, each on a stream of its own, x 0.1 s of signal per call (bench.py's block and
settings), timed with the feed off, with the programme audio meter on all channels (loud_kernel reads the same 157 MB of PCM: the yardstick for the block
kernel's rate), with the feed on one channel, and with it on all channels.  The method is tools/sca_bench.py's: device buffers, a stream of the tool's
own, a warm-up, then the mean over the timed calls; the modes alternate, --rounds times, in one job.  Prints one JSON line per round.

    python tools/feed_bench.py [--channels 4096] [--streams 4096] [--calls 20] [--warmup 5] [--rounds 2] [--modes off,loud_all,one,all] [--tree DIR]

added_ms_per_call_* is a mode's time less the off mode's of the same round; gbytes_per_s_* is the PCM the stage reads per call (channels x 4800 frames x
8 bytes) over that added time -- the stage runs alone on the call's stream behind stage C, so the added time is its kernels' time.  In mode all the ten
blocks a call completes per channel are then read once as 16 bit to the host (fmx_feed_read) and, behind one more call, once to a device tensor
(fmx_feed_read_device): read_*_ms.  --tree DIR takes the package and its library from another checkout: --modes off --tree <the parent commit's build>
times the same handle on the code without the feed, in the same job."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="off,loud_all,one,all")
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
    pcm_bytes = C * (n // 48) * 8
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    for _ in range(args.rounds):
        out = {"tree": "this" if os.path.abspath(args.tree) == ROOT else "other", "channels": C, "streams": S, "samples_per_call": n,
               "signal_seconds_per_call": 0.1, "calls": args.calls, "pcm_mbytes_per_call": round(pcm_bytes / 1e6, 1)}
        for mode in args.modes.split(","):
            f = pkg.Fmx(C, streams=S, stream_of_channel=[c % S for c in range(C)], device=0, max_block=n)
            for pid, v in ((m.P_BANDWIDTH, 165000), (m.P_LF_CUTOFF, 15000), (m.P_DEEMPHASIS, 50), (m.P_VOLUME_DB, -6.0)):
                f.set_param(pid, v)
            if mode == "loud_all":
                f.audio_meter(True)
            elif mode in ("one", "all"):
                f.feed(1, C // 2 if mode == "one" else -1)

            def call():
                f.process_device(iq.data_ptr(), n, n, pcm.data_ptr(), frames_cap, hip_stream=stream.cuda_stream)
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            torch.cuda.synchronize()
            out["ms_per_call_" + mode] = round((time.perf_counter() - t0) * 1e3 / args.calls, 4)
            out["second_group_" + mode] = f.last_second_group()
            if mode == "one":
                out["blocks_read_one"] = int(len(f.feed_read(C // 2, 1, capacity=10, power=False)[0][1]))
            if mode == "all":
                # the newest ten blocks per channel are what a reader behind every call takes: drop the older ones, then time one call's worth
                f.feed_read(0, C, capacity=128, power=False)
                call()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = f.feed_read(0, C, capacity=10, fmt="s16")
                out["read_s16_host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                out["blocks_read_all"] = int(sum(len(r[1]) for r in got))
                call()
                torch.cuda.synchronize()
                d_audio = torch.empty((C, 10 * m.FEED_BLOCK), dtype=torch.float32, device=dev)
                d_power = torch.empty((C, 10), dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs = f.feed_read(0, C, capacity=10, device=(d_audio, d_power, stream.cuda_stream))
                torch.cuda.synchronize()
                out["read_f32_device_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                out["blocks_read_device"] = int(sum(r[1] for r in runs))
            f.close()
        if "ms_per_call_off" in out:
            for mode in ("loud_all", "one", "all"):
                if "ms_per_call_" + mode in out:
                    added = out["ms_per_call_" + mode] - out["ms_per_call_off"]
                    out["added_ms_per_call_" + mode] = round(added, 4)
                    if mode != "one" and added > 0:
                        out["gbytes_per_s_" + mode] = round(pcm_bytes / (added * 1e-3) / 1e9, 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
