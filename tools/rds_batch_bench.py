"""What it costs to ask a batch for its RDS picture: 2048 channels with RDS_2 on, calls of 0.1 s (230400 input samples), config4's settings.
Per timed call: the step itself (fmx_process_device + synchronise), then (a) a loop of fmx_rds_decode over every channel -- one device synchronisation
and two blocking copies each, the synchroniser on the host over the bit ring -- and (b) one fmx_rds_decode_all -- the synchroniser has run on the GPU
in the step, one read-out, the group decoders on the host.  The C entries are timed directly (no Python list building).  Prints one JSON line.

    python tools/rds_batch_bench.py [--channels 2048] [--calls 10] [--warmup 15] [--no-loop]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--no-loop", action="store_true", help="skip (a): for a kernel-trace run of the step alone")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sdr-j-fm_amd")
    m = pkg.fmx
    n, nch, nst = 230400, args.channels, min(64, args.channels)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    iq = (torch.randn((nst, n, 2), generator=g, device=dev) * 0.1).contiguous()
    frames_cap = n // 48 + 96
    pcm = torch.zeros((nch, frames_cap, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    f = pkg.Fmx(nch, streams=nst, stream_of_channel=[c % nst for c in range(nch)], device=0, max_block=n)
    for pid, v in ((m.P_BANDWIDTH, 165000), (m.P_LF_CUTOFF, 15000), (m.P_DEEMPHASIS, 50), (m.P_VOLUME_DB, -6.0), (m.P_RDS_MODE, 2)):
        f.set_param(pid, v)
    infos = (m.FmxRdsInfo * nch)()
    one = m.FmxRdsInfo()

    def step():
        f.process_device(iq.data_ptr(), n, n, pcm.data_ptr(), frames_cap, hip_stream=stream.cuda_stream)
        torch.cuda.synchronize()

    def sweep_all():
        assert f.L.fmx_rds_decode_all(f.h, 0, nch, infos) == 0

    def sweep_loop():
        for c in range(nch):
            f.L.fmx_rds_decode(f.h, c, C.byref(one))

    for _ in range(args.warmup):
        step()
    sweep_all()
    if not args.no_loop:
        sweep_loop()
    t = {"step": [], "decode_all": [], "decode_loop": []}
    for _ in range(args.calls):
        t0 = time.perf_counter(); step()
        t1 = time.perf_counter(); sweep_all()
        t2 = time.perf_counter()
        if not args.no_loop:
            sweep_loop()
        t3 = time.perf_counter()
        t["step"].append(t1 - t0); t["decode_all"].append(t2 - t1); t["decode_loop"].append(t3 - t2)
    out = {"channels": nch, "block": n, "calls": args.calls, "bits_per_channel": int(len(f.rds_bits(0, 8192)))}
    for k, v in t.items():
        if k == "decode_loop" and args.no_loop:
            continue
        v = sorted(v)
        out["ms_" + k] = {"median": round(v[len(v) // 2] * 1e3, 4), "min": round(v[0] * 1e3, 4), "max": round(v[-1] * 1e3, 4)}
    same = sum(1 for c in range(nch) if bytes(infos[c])[:32] == bytes(f.rds_decode(c))[:32]) if not args.no_loop else None
    out["channels_with_equal_counters"] = same
    print(json.dumps(out))


if __name__ == "__main__":
    main()
