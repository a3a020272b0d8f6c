"""Scan mode's cost at batch scale: 4096 channels, bench.py's block (230400 input samples = 19200 fm samples per call), config4's settings.
Times 50 calls after a warm-up, first with no channel scanning, then with every channel scanning, and prints one JSON line.  The scan
kernel's own time comes from a separate kernel-trace run of this script (`--only scan`, under rocprofv3 --kernel-trace --stats).

    python tools/scan_bench.py [--channels 4096] [--calls 50] [--warmup 20] [--only both|none|scan]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="both", choices=["both", "none", "scan"])
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sdr-j-fm_amd")
    m = pkg.fmx
    n = 230400
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    iq = (torch.randn((args.channels, n, 2), generator=g, device=dev) * 0.1).contiguous()
    frames_cap = n // 48 + 96
    pcm = torch.zeros((args.channels, frames_cap, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    out = {"channels": args.channels, "block": n, "fm_samples_per_call": n // 12, "calls": args.calls}
    modes = {"both": ("none", "scan"), "none": ("none",), "scan": ("scan",)}[args.only]
    for mode in modes:
        f = pkg.Fmx(args.channels, device=0, max_block=n)
        for pid, v in ((m.P_BANDWIDTH, 165000), (m.P_LF_CUTOFF, 15000), (m.P_DEEMPHASIS, 50), (m.P_VOLUME_DB, -6.0)):
            f.set_param(pid, v)
        f.set_param(m.P_SCANNING, 1 if mode == "scan" else 0)
        for _ in range(args.warmup):
            f.process_device(iq.data_ptr(), n, n, pcm.data_ptr(), frames_cap, hip_stream=stream.cuda_stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            f.process_device(iq.data_ptr(), n, n, pcm.data_ptr(), frames_cap, hip_stream=stream.cuda_stream)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.calls
        out["ms_per_call_" + mode] = round(ms, 4)
        if mode == "scan":
            recs = f.scan_results(0)
            out["records_per_channel"] = int(len(recs))
            assert not pcm[:, :f.frames_for(n)].any().item(), "a scanning channel's PCM must be zeros"
        f.close()
    if "ms_per_call_none" in out and "ms_per_call_scan" in out:
        out["scan_cost_ms"] = round(out["ms_per_call_scan"] - out["ms_per_call_none"], 4)
    # what the scan kernel reads per call: 8 B per fm sample and channel
    out["scan_bytes_per_call"] = 8 * (n // 12) * args.channels
    print(json.dumps(out))


if __name__ == "__main__":
    main()
