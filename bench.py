#!/usr/bin/env python3
"""bench.py -- throughput of the FM demodulation hot path on MI355X (BASELINE.json metric:
"IQ MSamples/s demodulated to 48 kHz stereo").

A "step" = one pass of the whole chain (front-end FIR -> discriminator/pilot PLL/PSS -> audio FIR +
resampler) over one batch: `channels` independent FM channels x `block` complex samples each,
IQ already resident in HBM.  Default workload = BASELINE configs[3] -- 4096 independent channels with
configs[1]'s per-channel settings (stereo + PSS + de-emphasis + input FIR ON) -- which fits one GPU
(7.5 GB of IQ per step), so every rank runs all of it (weak scaling: 4096 channels per GPU); `--workload
shard512` is the same config split over eight GPUs.

Multi-GPU: one rank per GPU, channels sharded, NO collective on the data path.  `--gpus N` with N > 1 and no
torchrun environment re-executes this script under `python -m torch.distributed.run --nproc-per-node N` (RCCL); under
torchrun WORLD_SIZE must equal --gpus.  RCCL is used only either side of the path, in separately timed legs reported
next to the headline value: `gather` (every rank's PCM of one step to rank 0) and, for configs[2], `broadcast` (the
shared wide-band streams from rank 0).

A plain run does what the headline needs and nothing else: it sets up, warms up, times K steps, writes the last timed step's
PCM if --dump-outputs DIR is given, and prints the result line (`metric`, `value`, `unit`, `higher_is_better`, `dtype`,
`ms_per_step`, the configuration).  Everything else it measures or checks runs with --full:
  kernels_ms_per_step, roofline, pilot_pll   a separate untimed, profiled pass (HIP events per stage), the streaming-bandwidth
                 probe, and on rank 0 at N = 1 roofline.control (the f32 stage-A kernel on fresh handles)
  rds_check      configs[4]: the decoded RDS bits against the generator's
  gather         N > 1: one step's PCM of every rank to rank 0 over RCCL
and, on rank 0 at N = 1, the extra legs (extra keys; the headline `value` stays the HBM-resident run):
  sustained      the same step loop for >= --sustain seconds
  host_ingest    raw uint8 / float32 IQ from PINNED host memory, double-buffered: the copy of step k+1 overlaps the
                 processing of step k (PCIe-inclusive rates)
  host_call      latency of the single-receiver drop-in call: 1 channel, 16384 samples, fmx_process_host (in a process of its own)
  cpu_baseline   the oracle (a port) on the host cores; with oracle/_ref present also the reference's own leaf classes
  other_workloads, strong_scaling_projection   the other BASELINE configs and the shard sizes, each a `--full --quick` run of its own
--full --quick keeps the profiled pass, the probe and the checks and drops the extra legs and the control.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload config4|shard512|config1|config2|config3|config5]
                    [--dump-outputs DIR] [--full [--quick]]
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

INPUT_RATE = 2304000
BLOCK = 230400            # 0.1 s per channel per step; every synthetic tone is periodic in it
ALG_BYTES_STAGE_A = 8.0 + 8.0 / 12.0      # 8 B read + 8/12 B written per input sample
HBM_PEAK_GBPS = 8000.0                    # MI355X_MICROARCH.md: 8 TB/s spec

WORKLOADS = {
    # name: (channels per GPU, streams per GPU (0 = one per channel), description)
    "config4": (4096, 0, "configs[3] whole on each GPU: 4096 independent 2.304 MS/s channels, configs[1] settings "
                         "(stereo + PSS + de-emphasis 50us + input FIR 165 kHz + audio LPF 15 kHz)"),
    "shard512": (512, 0, "configs[3] split over 8 GPUs, one GPU's shard: 512 independent channels, configs[1] settings"),
    "config1": (4096, 0, "configs[0] at batch scale: 4096 channels, each with configs[0]'s settings (mono FM, input filter OFF, de-emphasis 50 us, "
                         "audio LPF 15 kHz): stage A then runs the 37-tap fold of the two decimators alone (front_kernel, packed f32 FMAs)"),
    "config2": (1, 0, "configs[1]: 1 channel, stereo + PSS + de-emphasis + input FIR ON"),
    "config3": (256, 24, "configs[2]: 256 carriers in 24 wide-band IQ streams (11 per stream, 200 kHz raster)"),
    "config5": (2048, 0, "configs[4] per-GPU shard: 2048 channels (16384 over 8 GPUs), full chain incl. the RDS front end and "
                        "RDS_2 bit slicer; the MPX carries a 57 kHz DSB-SC sub-carrier with 475 differentially encoded biphase bits "
                        "per channel, cyclically (four blocks of 0.1 s); the decoded bits are checked behind the timed region"),
}


DUMP_BYTES = 60 * 10 ** 6                 # --dump-outputs: at most this many bytes of PCM (a fixed sample of the channels beyond it)

RDS_BLOCKS = 4            # 4 blocks of 0.1 s = 475 RDS bits (1187.5 bit/s): the shortest run of blocks that is periodic in the bit clock
RDS_CYCLE_BITS = 475


def rds_cycle_bits(channel):
    """The 475 data bits channel `channel` of the config5 workload sends, cyclically (even parity, so that the differential
    encoder's state closes the cycle)."""
    b = np.random.default_rng(50000 + channel).integers(0, 2, RDS_CYCLE_BITS).astype(np.uint8)
    b[-1] ^= b.sum() & 1
    return b


def synth_device(torch, channels, n, device, offsets_hz=None, seed=0, rds_level=0.0, first_channel=0):
    """[channels, n, 2] float32 stereo-FM IQ on the GPU, periodic in n (all tones multiples of 10 Hz).  With rds_level > 0 the MPX
    carries a 57 kHz DSB-SC sub-carrier (in quadrature with the pilot's third harmonic) with differentially encoded biphase bits at
    1187.5 bit/s -- the oracle generator's modulation (oracle/fm_oracle.c fmo_siggen_run) -- and n must be RDS_BLOCKS blocks."""
    out = torch.empty((channels, n, 2), dtype=torch.float32, device=device)
    t = torch.arange(n, dtype=torch.float64, device=device) / INPUT_RATE
    g = torch.Generator(device="cpu").manual_seed(1234 + seed)
    step = 32
    for c0 in range(0, channels, step):
        c1 = min(channels, c0 + step)
        k = torch.arange(c0, c1, dtype=torch.float64)
        fl = (300 + 10 * ((37 * k) % 400)).to(device)[:, None]          # left tone, Hz
        fr = (500 + 10 * ((53 * k) % 400)).to(device)[:, None]
        ph = (torch.rand((c1 - c0, 3), generator=g, dtype=torch.float64) * 2 * np.pi).to(device)
        L = 0.5 * torch.sin(2 * np.pi * fl * t + ph[:, 0:1])
        R = 0.5 * torch.sin(2 * np.pi * fr * t + ph[:, 1:2])
        p19 = 2 * np.pi * 19000.0 * t + ph[:, 2:3]
        mpx = 0.45 * (L + R) + 0.10 * torch.sin(p19) + 0.45 * (L - R) * torch.sin(2 * p19)
        if rds_level > 0:
            assert n == RDS_BLOCKS * BLOCK
            bt = t * 1187.5
            kbit = torch.floor(bt).long().clamp_(max=RDS_CYCLE_BITS - 1)
            shape = torch.sin(2 * np.pi * (bt - kbit))                   # biphase: +half, then -half
            data = np.stack([rds_cycle_bits(first_channel + c) for c in range(c0, c1)])
            diff = np.bitwise_xor.accumulate(data, axis=1)                # differential encoding over the data bits
            sym = torch.as_tensor(diff.astype(np.float64) * 2 - 1, device=device)
            mpx = mpx + rds_level * torch.gather(sym, 1, kbit[None, :].expand(c1 - c0, -1)) * shape * torch.cos(3 * p19)
        off = 0.0 if offsets_hz is None else torch.as_tensor(offsets_hz[c0:c1], dtype=torch.float64, device=device)[:, None]
        inc = 2 * np.pi * (75000.0 * mpx + off) / INPUT_RATE
        inc = inc - inc.mean(dim=1, keepdim=True) * (0.0 if offsets_hz is not None else 1.0)   # exact periodicity
        phase = torch.cumsum(inc, dim=1)
        out[c0:c1, :, 0] = (0.5 * torch.cos(phase)).float()
        out[c0:c1, :, 1] = (0.5 * torch.sin(phase)).float()
    return out


POPULATIONS = {
    # name: (description, [(fraction, kind)])   kinds: est = established stereo station, noise = no station (complex white noise),
    # cnr17 = the station at 17 dB wide-band CNR, nopilot = a mono transmitter (no pilot, no L-R), flap = a station whose pilot comes and goes
    "established": ("every channel an established stereo station (pilot locked, PSS established): the headline's population", [(1.0, "est")]),
    "mixed": ("70 % established stereo, 10 % noise only, 10 % at 17 dB CNR, 5 % without pilot, 5 % with a pilot that comes (65 % of a 1 s cycle) "
              "and goes, the cycles of the channels shifted against each other", [(0.70, "est"), (0.10, "noise"), (0.10, "cnr17"), (0.05, "nopilot"), (0.05, "flap")]),
    "unlocked": ("no channel ever locks: half noise only, half mono transmitters without pilot", [(0.5, "noise"), (0.5, "nopilot")]),
}
FLAP_BLOCKS = 10          # the pilot's on / off cycle of the "flap" channels: 10 blocks of 0.1 s


def population_kinds(name, channels):
    """kind of every channel: the population's fractions dealt out so that the kinds interleave (channel c -> slot (37 c) mod 100)"""
    spec = POPULATIONS[name][1]
    edges, acc = [], 0.0
    for frac, kind in spec:
        acc += frac
        edges.append((acc * 100.0 - 1e-9, kind))
    kinds = []
    for c in range(channels):
        slot = (37 * c) % 100
        kinds.append(next(k for e, k in edges if slot < e))
    return kinds


def synth_population(torch, channels, n, nblk, device, kinds, seed=0):
    """[channels, nblk * n, 2] float32 IQ: per channel what its kind says (POPULATIONS), periodic in nblk * n samples.  Everything but the
    "flap" channels is one block repeated; a flap channel's pilot is on for 65 % of the nblk-block cycle, starting at a channel-specific
    point of it, with the FM phase continuous through the whole cycle."""
    out = torch.empty((channels, nblk * n, 2), dtype=torch.float32, device=device)
    g = torch.Generator(device="cpu").manual_seed(4321 + seed)
    gd = torch.Generator(device=device).manual_seed(99 + seed)
    sigma17 = float(np.sqrt(0.25 / (2 * 10 ** 1.7)))
    step = 16
    for c0 in range(0, channels, step):
        c1 = min(channels, c0 + step)
        kk = kinds[c0:c1]
        flap = [k == "flap" for k in kk]
        L_ = nblk * n if any(flap) else n
        t = torch.arange(L_, dtype=torch.float64, device=device) / INPUT_RATE
        k = torch.arange(c0, c1, dtype=torch.float64)
        fl = (300 + 10 * ((37 * k) % 400)).to(device)[:, None]
        fr = (500 + 10 * ((53 * k) % 400)).to(device)[:, None]
        ph = (torch.rand((c1 - c0, 4), generator=g, dtype=torch.float64)).to(device)
        L = 0.5 * torch.sin(2 * np.pi * fl * t + 2 * np.pi * ph[:, 0:1])
        R = 0.5 * torch.sin(2 * np.pi * fr * t + 2 * np.pi * ph[:, 1:2])
        p19 = 2 * np.pi * 19000.0 * t + 2 * np.pi * ph[:, 2:3]
        pil = torch.tensor([0.0 if x == "nopilot" else 0.10 for x in kk], dtype=torch.float64, device=device)[:, None]
        dsb = torch.tensor([0.0 if x == "nopilot" else 0.45 for x in kk], dtype=torch.float64, device=device)[:, None]
        pilot = pil * torch.sin(p19)
        if any(flap):
            cyc = torch.remainder(t[None, :] * (INPUT_RATE / float(nblk * n)) + ph[:, 3:4], 1.0)      # position in the on / off cycle
            on = (cyc < 0.65).to(torch.float64)
            fm = torch.tensor([1.0 if x else 0.0 for x in flap], dtype=torch.float64, device=device)[:, None]
            pilot = pilot * (1.0 - fm + fm * on)
        mpx = 0.45 * (L + R) + pilot + dsb * (L - R) * torch.sin(2 * p19)
        inc = 2 * np.pi * 75000.0 * mpx / INPUT_RATE
        inc = inc - inc.mean(dim=1, keepdim=True)
        phase = torch.cumsum(inc, dim=1)
        amp = torch.tensor([0.0 if x == "noise" else 0.5 for x in kk], dtype=torch.float64, device=device)[:, None]
        sig = torch.stack([(amp * torch.cos(phase)).float(), (amp * torch.sin(phase)).float()], dim=2)
        sg = torch.tensor([0.2 if x == "noise" else (sigma17 if x == "cnr17" else 0.0) for x in kk], dtype=torch.float32, device=device)[:, None, None]
        if float(sg.max()) > 0:
            sig[:, :n] += sg * torch.randn((c1 - c0, n, 2), generator=gd, dtype=torch.float32, device=device)    # (only the first block of a channel that is not a flap channel is kept)
        if L_ == n:
            out[c0:c1] = sig.repeat(1, nblk, 1)
        else:
            for i, f_ in enumerate(flap):
                out[c0 + i] = sig[i] if f_ else sig[i, :n].repeat(nblk, 1)
    return out


def usable_cores():
    """Host cores this process may really use: the affinity mask, cut down by a cgroup CPU quota if one is set."""
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // per))
            break
        except Exception:
            continue
    return n


def cpu_baseline(seconds_budget=12.0, ref_budget=6.0, config0_budget=5.0):
    """The oracle (a port of the reference chain, oracle/fm_oracle.c) timed on this box's host cores:
    one channel per core, all usable cores busy, configs[1] settings -- the reference is single-threaded per
    channel.  Bounded sample: every worker demodulates 0.1 s blocks until the time budget is spent.
    When oracle/_ref/libfmref.so travelled to this box, the reference's OWN leaf classes wired by ref_chain_run (up to
    the resampler input) are timed the same way beside it: the port is the faster of the two by about 10 %."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    cores = usable_cores()
    n = 16384 * 14                                    # ~0.1 s block, multiple of the reference's 16384
    iq = ol.synth_iq(n)
    L = ol.oracle()

    def timed(make, run, budget):
        objs = [make() for _ in range(cores)]
        done = [0] * cores
        t0 = time.perf_counter()

        def work(i):
            while True:
                run(objs[i], i)
                done[i] += 1
                if time.perf_counter() - t0 >= budget:
                    break

        th = [threading.Thread(target=work, args=(i,)) for i in range(cores)]
        for x in th: x.start()
        for x in th: x.join()
        return sum(done), time.perf_counter() - t0, objs

    pcm = [np.zeros((n // 48 + 64, 2), np.float32) for _ in range(cores)]
    blocks, dt, chains = timed(lambda: ol.OracleChain(inputFilterBw=165000),
                               lambda c, i: L.fmo_chain_process(c.h, ol.fptr(iq), n, ol.fptr(pcm[i]), pcm[i].shape[0]),
                               seconds_budget)
    total = blocks * n
    out = {"value": round(total / dt / 1e6, 3), "unit": "MS/s", "cores": cores, "kind": "port",
           "sample": "%d channels (one per usable core), %d blocks of %d samples in all within a %.0f s budget, "
                     "configs[1] settings, oracle/fm_oracle.c -O2" % (cores, blocks, n, seconds_budget),
           "per_core_MSps": round(total / dt / 1e6 / cores, 3)}
    del chains
    # SURVEY 8d asks for both CPU-runnable configs: configs[0] (mono FM, input filter OFF) beside configs[1]
    blocks0, dt0, chains = timed(lambda: ol.OracleChain(inputFilterBw=0, fmMode=2),
                                 lambda c, i: L.fmo_chain_process(c.h, ol.fptr(iq), n, ol.fptr(pcm[i]), pcm[i].shape[0]),
                                 config0_budget)
    out["configs0"] = {"value": round(blocks0 * n / dt0 / 1e6, 3), "unit": "MS/s", "cores": cores, "kind": "port",
                       "sample": "%d channels (one per usable core), %d blocks of %d samples in all within a %.0f s budget, configs[0] settings "
                                 "(mono FM, input filter OFF)" % (cores, blocks0, n, config0_budget)}
    del chains
    R = ol.ref()
    if R is not None and R.ref_has_qt():
        nf = n // 12 + 8
        outs = [np.zeros((nf, 2), np.float32) for _ in range(cores)]
        blocks, dt, objs = timed(lambda: R.ref_chain_new(2304000, 192000, 3, 165000, 15000, 50, -6.0, 0, 1, 1, 1, 0, 0),
                                 lambda c, i: R.ref_chain_run(c, ol.fptr(iq), n, None, None, None, ol.fptr(outs[i])),
                                 ref_budget)
        for c in objs:
            R.ref_chain_free(c)
        out["reference_leaf_chain_MSps"] = round(blocks * n / dt / 1e6, 3)
        out["reference_leaf_chain_note"] = ("the reference's own classes (oracle/_ref) wired by ref_chain_run, up to the resampler "
                                            "input, %d cores, %d blocks in %.0f s" % (cores, blocks, ref_budget))
    return out


def dump_outputs(d, torch, pcm, channels, frames):
    """--dump-outputs: the PCM the last timed step returned, [channels, frames, 2] float32, as d/pcm.npy -- all channels, or a fixed
    sample of them (seed 0, ascending, indices in d/pcm_channels.npy) when all would exceed DUMP_BYTES."""
    os.makedirs(d, exist_ok=True)
    k = min(channels, max(1, DUMP_BYTES // (frames * 2 * 4)))
    idx = np.arange(channels) if k == channels else np.sort(np.random.default_rng(0).choice(channels, k, replace=False))
    sel = torch.as_tensor(idx, dtype=torch.long, device=pcm.device)
    np.save(os.path.join(d, "pcm.npy"), pcm.index_select(0, sel)[:, :frames].cpu().numpy().astype(np.float32))
    np.save(os.path.join(d, "pcm_channels.npy"), idx.astype(np.float64))


def sub_bench(extra):
    """One short run of this script in a process of its own (another workload / shard size); returns the compact result."""
    cmd = [sys.executable, os.path.abspath(__file__), "--full", "--quick"] + extra
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ))
        j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        k = j["kernels_ms_per_step"]
        return {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "channels_per_gpu": j["config"]["channels_per_gpu"],
                "front_kernel_used": j.get("front_kernel_used"),
                "kernels_ms_per_step": {x: k[x] for x in ("front_fir", "demod_pilot_pss", "audio_fir_resample")},
                "stage_b_min_median_max": j["kernels_ms_per_step_raw"]["stage_b_min_median_max"], "pilot_pll": j["pilot_pll"],
                **({"call_pieces": j["call_pieces"]["pieces_per_call"]} if "call_pieces" in j else {}),
                "front_fir_frac_of_8TBps": j["roofline"]["frac"], **({"front_fir_bytes": j["roofline"]["front_fir_bytes"]} if "front_fir_bytes" in j["roofline"] else {}),
                **({"rds_check": j["rds_check"]} if "rds_check" in j else {})}
    except Exception as e:          # an extra leg must not take the headline line down
        return {"error": "%s: %s" % (type(e).__name__, e)}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def respawn(args, argv):
    """--gpus N without a torchrun environment: run N ranks of this script under torch.distributed.run."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "1"))
    return subprocess.call(cmd, env=env)


def selftest_spawn(args):
    """CPU check of the N > 1 plumbing (tests/test_bench_spawn.py): the spawned ranks meet over gloo, run the timing
    reduction and the gather leg on host tensors, and rank 0 prints a line with the same keys.  Measures nothing."""
    import torch
    import torch.distributed as dist
    world = int(os.environ["WORLD_SIZE"]); rank = int(os.environ["RANK"])
    dist.init_process_group(backend="gloo")
    shard = importlib.import_module("sdr-j-fm_amd").shard
    dt = shard.max_over_ranks(0.5 + 0.25 * rank)
    ch = 3
    pcm = torch.full((ch, 8, 2), float(rank))
    t0 = time.perf_counter()
    full = shard.gather_pcm(pcm, world * ch, dst=0)
    g_ms = (time.perf_counter() - t0) * 1e3
    vals = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(vals, torch.tensor([float(rank)], dtype=torch.float64))
    if rank == 0:
        assert full.shape[0] == world * ch and all(float(full[r * ch, 0, 0]) == r for r in range(world))
        print(json.dumps({"selftest": True, "metric": "IQ MSamples/s demodulated to 48 kHz stereo", "value": None, "n_gpus": world,
                          "rccl_ranks": dist.get_world_size(), "rccl_backend": dist.get_backend(),
                          "steps": args.steps, "warmup": args.warmup, "max_dt": dt, "scaling": "weak",
                          "per_rank": [float(v.item()) for v in vals], "gather": {"ms": round(g_ms, 3)}}))
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=12)   # (at least 44 untimed calls are made: see the timed region)
    ap.add_argument("--workload", default="config4", choices=sorted(WORKLOADS))
    ap.add_argument("--channels", type=int, default=0, help="override channels per GPU")
    ap.add_argument("--population", default="established", choices=sorted(POPULATIONS),
                    help="what the channels of a one-stream-per-channel workload receive (POPULATIONS); the headline is `established`")
    ap.add_argument("--decoder", type=int, default=0, help="fm_Demodulator::setDecoder for every channel (1 AM 2 PLL 3 Mixed ... 6 Diff; 0: the default, Mixed)")
    ap.add_argument("--pll-solver", type=int, default=0, help="FMX_P_PLL_SOLVER for every channel (0: the handle's default)")
    ap.add_argument("--squelch", type=int, default=0, help="set_squelchMode for every channel (1 noise squelch, 2 level squelch)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: every rank runs the workload's channel count; strong: --total-channels split over the ranks "
                         "(shard.shard_channels), BASELINE configs[3] literally: 4096 channels over 1/2/4/8 GPUs")
    ap.add_argument("--total-channels", type=int, default=0, help="strong scaling: channels of the whole job (default: the workload's count)")
    ap.add_argument("--no-extra-workloads", action="store_true", help="skip the one-line runs of the other BASELINE configs and shard sizes")
    ap.add_argument("--block", type=int, default=BLOCK)
    ap.add_argument("--sustain", type=float, default=5.0, help="seconds of the sustained leg (0 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ingest", action="store_true", help="skip the host-ingest and host-call legs")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: the profiled pass (kernels_ms_per_step, roofline), the bandwidth probe, the checks, "
                         "and the extra legs (sustained / ingest / latency / CPU / control / other workloads)")
    ap.add_argument("--quick", action="store_true", help="with --full: no sustained / ingest / latency / CPU / control / other-workload legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the PCM of the last timed step as DIR/pcm.npy (float32 [channels, frames, 2]; a fixed sample of the channels "
                         "when all would exceed %d MB, their indices in DIR/pcm_channels.npy)" % (DUMP_BYTES // 10 ** 6))
    ap.add_argument("--stride-pad", type=int, default=0,
                    help="complex samples of padding between consecutive streams in the IQ buffer (even)")
    ap.add_argument("--selftest-spawn", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--host-call-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.host_call_only:                      # the host_call leg's own process: a receiver's, nothing else on the device
        print(json.dumps(host_call_latency(importlib.import_module("sdr-j-fm_amd"), int(os.environ.get("LOCAL_RANK", "0")))))
        return
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if not args.full:                            # a plain run: the headline only
        args.quick = True
    if args.quick:
        args.sustain = 0.0; args.no_ingest = True; args.no_cpu_baseline = True; args.no_extra_workloads = True

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(respawn(args, sys.argv[1:]))
    world = int(env_world) if env_world is not None else 1
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node equal to --gpus "
                         "(or without torchrun, bench.py spawns the ranks itself)" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.selftest_spawn:
        return selftest_spawn(args)

    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: libfmx has no CPU fallback")
    if local_rank >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d has no GPU (%d visible, --gpus %d)" % (local_rank, torch.cuda.device_count(), args.gpus))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=device)

    fmx_amd = importlib.import_module("sdr-j-fm_amd")
    m = fmx_amd.fmx
    shard = fmx_amd.shard
    channels, streams, desc = WORKLOADS[args.workload]
    if args.channels > 0:
        channels = args.channels
    total_channels = world * channels
    first_channel = rank * channels
    if args.scaling == "strong":
        if streams:
            raise SystemExit("bench.py: --scaling strong is defined for the one-stream-per-channel workloads")
        total_channels = args.total_channels if args.total_channels > 0 else channels
        first_channel, channels = shard.shard_channels(total_channels, world, rank)
        if channels < 1:
            raise SystemExit("bench.py: fewer channels than ranks")
    rank_channels = [shard.shard_channels(total_channels, world, r)[1] if args.scaling == "strong" else channels for r in range(world)]
    n = args.block
    smap = None
    if streams:
        # configs[2]: channel c listens to carrier (c % 11) of stream c // 11 via set_localOscillator
        smap = [min(c // 11, streams - 1) for c in range(channels)]
    nstreams = streams if streams else channels
    nblk = 1                  # blocks of n samples per stream in the IQ buffer (the calls walk through them cyclically)

    def configure(f, nch):
        f.set_param(m.P_BANDWIDTH, 0 if args.workload == "config1" else 165000)
        f.set_param(m.P_LF_CUTOFF, 15000)
        f.set_param(m.P_DEEMPHASIS, 50)
        f.set_param(m.P_VOLUME_DB, -6.0)
        f.set_param(m.P_FM_MODE, 2 if args.workload == "config1" else 0)
        if args.workload == "config5":
            f.set_param(m.P_RDS_MODE, 2)
        if args.pll_solver:
            f.set_param(m.P_PLL_SOLVER, args.pll_solver)
        if args.decoder:
            f.set_param(m.P_FM_DECODER, args.decoder)
        if args.squelch:
            f.set_param(m.P_SQUELCH_MODE, args.squelch)
            f.set_param(m.P_SQUELCH_VALUE, 30)
        if streams:
            for c in range(nch):
                f.set_param(m.P_LOCAL_OSCILLATOR, ((c % 11) - 5) * 200000, channel=c)

    f = fmx_amd.Fmx(channels, streams=streams, stream_of_channel=smap, device=local_rank, max_block=n)
    configure(f, channels)

    bcast = None
    if streams:
        # 11 carriers per wide-band stream on a 200 kHz raster; the streams are SHARED by all ranks (every rank demodulates
        # its own carriers out of the same samples): rank 0 synthesises, RCCL broadcasts (the fan-out leg of SURVEY 8e)
        iq = torch.zeros((nstreams, n, 2), dtype=torch.float32, device=device)
        if rank == 0:
            for k in range(11):
                offs = [((k - 5) * 200000.0)] * nstreams
                iq += synth_device(torch, nstreams, n, device, offsets_hz=offs, seed=k) * (1.0 / 3.5)
        if world > 1:
            torch.cuda.synchronize(); dist.barrier()
            t0 = time.perf_counter()
            shard.broadcast_stream(iq, src=0)
            torch.cuda.synchronize()
            bt = time.perf_counter() - t0
            bcast = {"ms": round(bt * 1e3, 3), "MB": round(iq.numel() * 4 / 1e6, 1), "GBps": round(iq.numel() * 4 / bt / 1e9, 2),
                     "what": "%d shared wide-band streams x %d samples from rank 0 to every rank (RCCL broadcast, first call: "
                             "includes communicator warm-up)" % (nstreams, n)}
    elif args.workload == "config5":
        nblk = RDS_BLOCKS
        iq = synth_device(torch, channels, nblk * n, device, seed=rank if args.scaling == "weak" else 1000 + first_channel,
                          rds_level=0.05, first_channel=first_channel)
    elif args.population != "established":
        kinds = population_kinds(args.population, channels)
        nblk = FLAP_BLOCKS if "flap" in kinds else 1
        iq = synth_population(torch, channels, n, nblk, device, kinds, seed=rank)
    else:
        iq = synth_device(torch, channels, n, device, seed=rank if args.scaling == "weak" else 1000 + first_channel)
    stride = nblk * n + args.stride_pad
    if args.stride_pad:
        padded = torch.zeros((nstreams, stride, 2), dtype=torch.float32, device=device)
        padded[:, :nblk * n] = iq
        iq = padded
    frames_cap = n // 48 + 96
    pcm = torch.zeros((channels, frames_cap, 2), dtype=torch.float32, device=device)
    # The call runs on a stream of the caller's own (what a host application passes).  torch's current stream here is HIP's
    # default stream, i.e. handle 0 = NULL, which the C ABI reads as "the handle's own stream, ordered behind the default
    # stream" -- correct, but the default stream's implicit synchronisation with other streams costs ~0.4 ms per call.
    call_stream = torch.cuda.Stream(device=device)
    call_stream.wait_stream(torch.cuda.current_stream())
    stream = call_stream.cuda_stream

    calls = [0]
    if os.environ.get("FMX_BENCH_PTRS"):         # (diagnostic: where the caller-side buffers landed)
        print("ptrs iq %#x pcm %#x" % (iq.data_ptr(), pcm.data_ptr()), file=sys.stderr)

    def step():
        k = calls[0] % nblk
        calls[0] += 1
        return f.process_device(iq.data_ptr() + k * n * 8, stride, n, pcm.data_ptr(), frames_cap, hip_stream=stream)

    def barrier():
        if world > 1:
            dist.barrier()

    # W untimed steps as asked -- and never fewer than 44: the synthetic signal's pilot lock arrives in calls 5-8 and the PSS state
    # machine declares its error minimised 3 s later (calls 36-40, stereo-separation.cpp:96-107); the calls around both transitions take
    # the state machines' slow paths (rocprofv3, per dispatch: stage B 3.3 / 2.7 / 2.4 / 2.2 / 2.3 ms there against 2.0-2.1), and the metric is
    # about the established state: pilot locked, PSS established (the headline must not depend on W)
    untimed = max(args.warmup, 44)
    for _ in range(untimed):
        step()
    torch.cuda.synchronize()
    f.synchronize()
    # ---- the timed region: exactly K steps, no profiling events inside ---------------------------------------------
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frames = 0
    for _ in range(args.steps):
        last_frames = step()
        frames += last_frames
    torch.cuda.synchronize()
    barrier()
    dt_local = time.perf_counter() - t0
    f.synchronize()                     # raises if a stage-B wait gave up during the run (the figures would be void)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, torch, pcm, channels, last_frames)
    dt = dt_local
    per_rank = [dt_local]
    if world > 1:
        tt = torch.tensor([dt_local], dtype=torch.float64, device=device)
        allt = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(allt, tt)
        per_rank = [float(x.item()) for x in allt]
        dt = max(per_rank)

    # ---- --full: per-kernel times from a separate, untimed pass (HIP events on the call's stream, recorded by the library) ----
    # Every profiled step is enqueued while a spin kernel holds the stream (~1 ms), so that the GPU meets the step's kernels and
    # events back to back: the intervals then hold kernel time only, not the host's enqueue gaps (which made the stage times of
    # the small workloads add up to more than ms_per_step).
    pieces = f.last_call_pieces()
    if args.full:
        f.profile_enable(True)
        f.profile_read(reset=True)
        prof = {"launches": [0, 0, 0, 0], "ms": [0.0, 0.0, 0.0, 0.0]}
        per_step = [[], [], []]                 # stage times of every profiled step (the populations in which they differ from step to step)
        rep0, ex0 = f.pll_replays(), f.pll_exact_segments()
        nprof = min(args.steps, 10) if nblk == 1 else max(min(args.steps, 10), nblk)     # (a whole cycle of the input blocks)
        for _ in range(nprof):
            with torch.cuda.stream(call_stream):
                torch.cuda._sleep(2000000)
            step()
            torch.cuda.synchronize()
            one = f.profile_read(reset=True)
            # (a call made in overlapping pieces -- FMX_P_CALL_PIECES: pre-pass batches -- records one set of events per piece: a step's stage time is their sum)
            pieces = f.last_call_pieces()
            for k in range(3):
                prof["launches"][k] += one["launches"][k] if pieces <= 1 else 1; prof["ms"][k] += one["ms"][k]
                per_step[k].append(one["ms"][k] / (max(one["launches"][k], 1) if pieces <= 1 else 1))
        torch.cuda.synchronize()
        pll_counts = {"steps": nprof, "fail_safe_replays_per_step": round((f.pll_replays() - rep0) / nprof, 2),
                      "guard_sequential_segments_per_step": round((f.pll_exact_segments() - ex0) / nprof, 1),
                      "segments_per_step": channels * -(-(n // 12) // 1536)}
        f.profile_enable(False)

    # ---- gather leg: one step's PCM of every rank to rank 0 over RCCL, timed on its own ------------------
    gather = None
    if world > 1 and args.full:
        fr = frames // max(args.steps, 1)
        loc = pcm[:, :fr].contiguous()
        shard.gather_pcm(loc, total_channels, dst=0)                # communicator / buffer warm-up
        torch.cuda.synchronize(); barrier()
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            shard.gather_pcm(loc, total_channels, dst=0)
        torch.cuda.synchronize(); barrier()
        gt = (time.perf_counter() - t0) / reps
        nbytes = (total_channels - channels) * fr * 2 * 4
        gather = {"ms_per_step": round(gt * 1e3, 3), "MB_per_step": round(nbytes / 1e6, 2), "GBps": round(nbytes / gt / 1e9, 2),
                  "what": "PCM of one step (%d channels x %d frames per rank) gathered on rank 0 (RCCL gather); not part of "
                          "`value`" % (channels, fr)}

    # ---- sustained leg: the same loop for >= --sustain seconds ------------------------------------------------------
    sustained = None
    if args.sustain > 0:
        barrier(); torch.cuda.synchronize()
        k = 0
        t0 = time.perf_counter()
        while True:
            for _ in range(10):
                step()
            k += 10
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            flag = torch.tensor([1.0 if el >= args.sustain else 0.0], device=device)
            if world > 1:
                dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            if flag.item() > 0:
                break
        barrier()
        el = time.perf_counter() - t0
        f.synchronize()
        if world > 1:
            tt = torch.tensor([el], dtype=torch.float64, device=device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = float(tt.item())
        sustained = {"seconds": round(el, 3), "steps": k, "value": round(float(total_channels) * n * k / el / 1e6, 3),
                     "unit": "MS/s", "ms_per_step": round(el / k * 1e3, 4)}

    rds_check = None
    if args.full and args.workload == "config5":
        # the decoded bit string of a few channels against what the generator sent (cyclic, 475 bits)
        torch.cuda.synchronize()
        worst, checked, nb = 0, 0, 0
        for c in sorted({0, 1, channels // 3, channels - 1}):
            got = f.rds_bits(c, 8192)[-1425:]
            want = rds_cycle_bits(first_channel + c)
            if len(got) < 1425:
                worst = max(worst, 1425); continue
            errs = min(int(np.count_nonzero(got != np.tile(want, 4)[lag:lag + 1425])) for lag in range(RDS_CYCLE_BITS))
            worst = max(worst, errs); checked += 1; nb = len(got)
        rds_check = {"channels_checked": checked, "bits_compared_per_channel": nb, "worst_bit_errors": worst,
                     "calls": calls[0], "what": "last 1425 decoded bits (three cycles) of the channels against the generator's cyclic bit string, best lag"}
        if world > 1:
            tt = torch.tensor([float(worst)], device=device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            rds_check["worst_bit_errors"] = int(tt.item())

    out = None
    if rank == 0:
        total = float(total_channels) * n * args.steps
        value = total / dt / 1e6
        front_kernel_used = f.last_front_kernel()       # which of the three stage-A kernels the handle ran (include/fmx.h: FMX_P_FRONT_KERNEL)
        # algorithmic bytes of ONE front-end launch: every channel reads its n samples (8 B) and writes n/12 (8 B)
        alg_bytes = ALG_BYTES_STAGE_A * channels * n
        out = {
            "metric": "IQ MSamples/s demodulated to 48 kHz stereo",
            "value": round(value, 3), "unit": "MS/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            # what the process group saw, not what the environment said (1 / none without a process group): the evidence that N ranks joined
            "rccl_ranks": dist.get_world_size() if world > 1 else 1, "rccl_backend": dist.get_backend() if world > 1 else None,
            "untimed_calls": untimed,
            "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None,
            # the arithmetic the path computes in: f32 throughout -- except that front4_kernel multiplies 3-term split-f16 operands on the matrix pipe
            # (22-bit operands behind a per-tile power-of-two scale, products exact, f32 accumulate: DESIGN 3.1); `roofline.control` holds the f32 kernel beside it
            "dtype": "f32 (stage A: 3-term split-f16 MFMA with a per-tile block exponent, f32 accumulate)" if front_kernel_used == 3 else "f32",
            "front_kernel_used": front_kernel_used, "data": "synthetic",
            "config": {"workload": args.workload, "description": desc, "population": args.population, "population_description": POPULATIONS[args.population][0],
                       "channels_per_gpu": channels, "channels_total": total_channels,
                       "streams_per_gpu": nstreams, "block_samples_per_channel": n,
                       "realtime_channels_equiv": round(value / 2.304, 1),
                       "pcm_frames_per_channel_per_step": frames // max(args.steps, 1), "parallelism": "channels sharded, 1 rank/GPU"},
        }
        if args.full:
            launches = max(prof["launches"][0], 1)
            ms_a = prof["ms"][0] / launches
            achieved = alg_bytes / (ms_a * 1e-3) / 1e9 if ms_a > 0 else 0.0
            # HBM bytes per launch from the rocprofv3 PMC passes (FETCH_SIZE doubled: gfx950 counts half the bytes of wide streaming reads; + WRITE_SIZE),
            # committed under profiles/; only valid for the configuration it was collected on.
            traffic = None
            try:
                pmcs = sorted(x for x in os.listdir(os.path.join(ROOT, "profiles")) if x.endswith("_front_pmc.json"))
                pmc = json.load(open(os.path.join(ROOT, "profiles", pmcs[-1])))
                if pmc.get("channels") == channels and pmc.get("block") == n:
                    traffic = pmc["front_kernel_hbm_bytes_per_launch"]
            except Exception:
                traffic = None
            # practical ceiling next to the nominal peak: this box's streaming bandwidth, measured after the timed
            # region with the library's probe kernels (float2 copy; and stage A's own shape: read 12, write 1)
            measured = {}
            try:
                import ctypes as C
                L = fmx_amd.load_library()
                L.fmx_debug_stream_bandwidth.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_double)]
                for mode, key in ((0, "copy_GBps"), (1, "read12_write1_GBps"), (2, "read_only_GBps")):
                    g = C.c_double()
                    # (over 7.5 GiB, the size of a step's input: a 1 GiB probe, rounds 2-5, re-read a buffer of which the 256 MB memory-side cache
                    # keeps a quarter from one pass to the next and reported 6.3 TB/s for a traffic mix that streams at 5.4-5.5,
                    # tools/ubench/stream_shape.hip)
                    if L.fmx_debug_stream_bandwidth(local_rank, mode, 15 << 29, 3, C.byref(g)) == 0:
                        measured[key] = round(g.value, 1)
            except Exception as e:      # the probe is a diagnostic; the bench line does not depend on it
                measured = {"error": str(e)}
            # the stage table as a decomposition of the timed step: the event intervals of the profiled pass, scaled so that they add up to
            # ms_per_step (the raw intervals stay beside it)
            raw = [prof["ms"][k] / max(prof["launches"][k], 1) for k in range(3)]
            ms_step = dt / args.steps * 1e3
            scale = ms_step / sum(raw) if sum(raw) > 0 else 1.0
            kernels_ms = {"front_fir": round(raw[0] * scale, 4), "demod_pilot_pss": round(raw[1] * scale, 4), "audio_fir_resample": round(raw[2] * scale, 4),
                          "scale": round(scale, 4), "note": "raw event intervals x scale = a decomposition of ms_per_step"}
            out.update({
                "roofline": {"bound": "hbm", "kernel": {1: "fmx::front_kernel", 3: "fmx::f4::front4_kernel"}.get(front_kernel_used, "?") + " (input FIR stage)",
                             "achieved": round(achieved, 2),
                             "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4),
                             "frac_read_only": round(achieved * (8.0 / ALG_BYTES_STAGE_A) / HBM_PEAK_GBPS, 4),
                             "traffic": traffic, "avg_launch_ms": round(ms_a, 4),
                             # both byte counts: what the channels consume (every channel reads its stream) and what is unique in HBM
                             # (a stream several channels listen to is read once from HBM, then from the caches)
                             "front_fir_bytes": {"per_channel_sample": alg_bytes, "unique_stream": 8.0 * nstreams * n + (8.0 / 12.0) * channels * n,
                                                 "frac_unique_stream": round((8.0 * nstreams * n + (8.0 / 12.0) * channels * n) / (ms_a * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if ms_a > 0 else None},
                             "algorithmic_bytes_per_launch": alg_bytes, "measured_stream_bandwidth": measured,
                             "frac_of_measured": (round(achieved / measured["read12_write1_GBps"], 4)
                                                  if measured.get("read12_write1_GBps") else None),
                             # (the read-12-write-1 probe is a kernel of its own shape, not a ceiling -- stage A beats it by 2-15 % --; what nothing beats is this
                             # GPU's read-only stream: the stage's READ rate against it)
                             "frac_read_only_of_measured_reads": (round(achieved * (8.0 / ALG_BYTES_STAGE_A) / measured["read_only_GBps"], 4)
                                                                  if measured.get("read_only_GBps") else None)},
                "kernels_ms_per_step": kernels_ms,
                "kernels_ms_per_step_raw": {"front_fir": round(raw[0], 4), "demod_pilot_pss": round(raw[1], 4), "audio_fir_resample": round(raw[2], 4),
                                            "stage_b_min_median_max": [round(float(v), 4) for v in (np.min(per_step[1]), np.median(per_step[1]), np.max(per_step[1]))],
                                            "note": "HIP-event intervals of a separate untimed pass of %d steps, each enqueued behind a spin kernel; their sum "
                                                    "exceeds the timed step by the events' own cost" % launches},
                "pilot_pll": pll_counts,
            })
        out.update({
            **({"stage_groups": {"channels": [channels - f.last_second_group(), f.last_second_group()],
                                 "note": "stages B and C run as two channel groups on two streams (the audio stage of one beside the stereo stage of the other); stage A, "
                                         "the roofline's kernel, is one launch with the chip to itself; the demod_pilot_pss interval ends with the first group's stage B"}}
               if f.last_second_group() > 0 else {}),
            **({"call_pieces": {"pieces_per_call": pieces, "note": "FMX_P_CALL_PIECES: the call is made in pieces whose stages overlap on three streams (stage A of piece k + 1, the "
                                "demodulator's lone-wave recurrences of piece k, stage B / C of piece k - 1); the stage intervals are sums over the pieces and overlap in time"}}
               if pieces > 1 else {}),
            "per_rank_value": [round(rank_channels[r] * n * args.steps / t / 1e6, 3) for r, t in enumerate(per_rank)],
        })
        if rds_check: out["rds_check"] = rds_check
        if gather: out["gather"] = gather
        if bcast: out["broadcast"] = bcast
        if sustained: out["sustained"] = sustained

    # ---- the f32 control of the headline's stage A: one extra untimed pass, rank 0 at N = 1 only ----------------------
    # Two fresh handles on the same input -- the automatic kernel choice (the matrix-pipe filter) and front_kernel forced (plain f32 packed FMAs) -- walk
    # the same calls from the stream's start through pilot lock; the last call's PCM of every channel is compared sample by sample, and front_kernel's
    # mean launch time is taken from the library's events as the headline's is.
    if rank == 0 and world == 1 and not args.quick and front_kernel_used == 3:
        del f
        f = None
        torch.cuda.empty_cache()
        try:
            ncalls = 12
            res = []
            for kern in (0, 1):
                fc = fmx_amd.Fmx(channels, streams=streams, stream_of_channel=smap, device=local_rank, max_block=n)
                configure(fc, channels)
                fc.set_param(m.P_FRONT_KERNEL, kern)
                pc = torch.zeros((channels, frames_cap, 2), dtype=torch.float32, device=device)
                fr = 0
                for k in range(ncalls):
                    if k == ncalls - 4:
                        torch.cuda.synchronize(); fc.profile_enable(True); fc.profile_read(reset=True)
                    fr = fc.process_device(iq.data_ptr() + (k % nblk) * n * 8, stride, n, pc.data_ptr(), frames_cap, hip_stream=stream)
                torch.cuda.synchronize()
                pr = fc.profile_read(reset=True)
                res.append((pc[:, :fr].clone(), pr["ms"][0] / max(pr["launches"][0], 1), fc.last_front_kernel()))
                del fc, pc
                torch.cuda.empty_cache()
            (pa, ms3, k3), (pb, ms1, k1) = res
            out["roofline"]["control"] = {"kernel": "fmx::front_kernel (f32 packed FMAs)" if k1 == 1 else "?", "avg_launch_ms": round(ms1, 4),
                                          "frac": round(alg_bytes / (ms1 * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if ms1 > 0 else None,
                                          "headline_kernel_avg_launch_ms_same_pass": round(ms3, 4), "headline_kernel": k3,
                                          "pcm_max_abs_diff": float((pa - pb).abs().max().item()), "pcm_rms_diff": float((pa - pb).double().pow(2).mean().sqrt().item()),
                                          "pcm_full_scale": float(pb.abs().max().item()),
                                          "what": "two fresh handles, the same %d calls from the stream's start (through pilot lock); PCM of the last call, every channel, "
                                                  "max and rms of |matrix-pipe stage A - f32 stage A| (call 12 sits behind the pilot's lock-in, where the stereo decoder has just switched on: the largest "
                                                  "differences are single samples there); launch times: mean of the last 4 calls" % ncalls}
            del pa, pb, res
        except Exception as e:      # the control is a report; the headline does not depend on it
            out["roofline"]["control"] = {"error": str(e)[:200]}
        torch.cuda.empty_cache()

    # ---- host-side legs, rank 0 at N = 1 only ---------------------------------------------------------------------------
    if rank == 0 and world == 1 and not args.no_ingest:
        if f is not None:
            del f
        torch.cuda.empty_cache()
        out["host_ingest"] = host_ingest_legs(torch, fmx_amd, configure, args, device, local_rank, n, streams, smap)
        out["host_call"] = host_call_leg(fmx_amd, local_rank)
    if rank == 0:
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
            if sustained:
                out["cpu_baseline"]["note"] = ("the port is ~10 %% faster than the reference's own classes; GPU/CPU ratio of "
                                               "the headline value = %.0f" % (out["value"] / out["cpu_baseline"]["value"]))
        if (world == 1 and not args.no_extra_workloads and args.workload == "config4" and args.channels == 0 and args.scaling == "weak"
                and args.population == "established" and not args.decoder and not args.squelch):
            # the other BASELINE configs as one-liners (so that the driver's record carries every config), and the shard sizes of
            # configs[3] split 2 / 4 / 8 ways: what strong scaling of 4096 channels comes to per GPU, before any RCCL cost (there is
            # no collective on the data path; `python bench.py --gpus N --scaling strong --total-channels 4096` measures it for real)
            out["other_workloads"] = {"configs[0] at batch scale (4096 channels, mono, input filter off)": sub_bench(["--workload", "config1"]),
                                      "configs[1] (1 channel)": sub_bench(["--workload", "config2"]),
                                      "configs[2] (256 carriers on 24 shared streams)": sub_bench(["--workload", "config3"]),
                                      "configs[4] shard (2048 channels, RDS on)": sub_bench(["--workload", "config5"]),
                                      # the path where it is slow: populations that are not all established, and the decoders /
                                      # squelch that run one lane per channel (fmx_demod.hip)
                                      "configs[3], mixed population": sub_bench(["--population", "mixed"]),
                                      "configs[3], no channel locked": sub_bench(["--population", "unlocked"]),
                                      "configs[3], PLL decoder on every channel": sub_bench(["--decoder", "2"]),
                                      "configs[3], noise squelch on every channel": sub_bench(["--squelch", "1"]),
                                      "configs[3], level squelch on every channel": sub_bench(["--squelch", "2"])}
            proj = {"1": {"channels_per_gpu": channels, "per_gpu_value": out["value"], "efficiency": 1.0}}
            for g in (2, 4, 8):
                r = sub_bench(["--channels", str(channels // g)])
                if "value" in r:
                    proj[str(g)] = {"channels_per_gpu": channels // g, "per_gpu_value": r["value"], "ms_per_step": r["ms_per_step"],
                                    "efficiency": round(r["value"] / out["value"], 4)}
                else:
                    proj[str(g)] = r
            out["strong_scaling_projection"] = {"what": "configs[3] (4096 channels in all) over N GPUs: one GPU's shard measured on this GPU; "
                                                        "efficiency = per-GPU rate of the shard / per-GPU rate at 4096 channels", "gpus": proj}
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def host_ingest_legs(torch, fmx_amd, configure, args, device, local_rank, n, streams, smap):
    """IQ from PINNED host memory through the raw device entry point, double-buffered on two HIP streams: the H2D copy of
    step k+1 runs while step k is processed (what an ingest process that owns the device ring does).  uint8 at the
    workload's channel count, float32 at a quarter of it (4x the bytes per sample)."""
    m = fmx_amd.fmx
    res = {}
    base_ch, _, _ = WORKLOADS[args.workload]
    if args.channels > 0:
        base_ch = args.channels
    for name, fmt, dtype, div in (("u8", m.IQ_U8, torch.uint8, 1), ("f32", m.IQ_F32, torch.float32, 4)):
        if streams:
            break                                   # shared-stream layout: the ingest figure is quoted on independent channels
        ch = max(1, base_ch // div)
        try:
            f = fmx_amd.Fmx(ch, device=local_rank, max_block=n)
            configure(f, ch)
            if fmt == m.IQ_U8:
                host = torch.randint(96, 160, (ch, n, 2), dtype=torch.uint8).pin_memory()
            else:
                host = (torch.rand((ch, n, 2), dtype=torch.float32) - 0.5).pin_memory()
            dev = [torch.empty((ch, n, 2), dtype=dtype, device=device) for _ in range(2)]
            pcm = torch.zeros((ch, n // 48 + 96, 2), dtype=torch.float32, device=device)
            s_copy, s_run = torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)
            ev_copied = [torch.cuda.Event() for _ in range(2)]
            ev_used = [torch.cuda.Event() for _ in range(2)]
            import ctypes as C
            L = f.L

            def run(steps):
                got = C.c_int64()
                for k in range(steps):
                    b = k & 1
                    with torch.cuda.stream(s_copy):
                        if k >= 2:
                            s_copy.wait_event(ev_used[b])
                        dev[b].copy_(host, non_blocking=True)
                        ev_copied[b].record(s_copy)
                    s_run.wait_event(ev_copied[b])
                    rc = L.fmx_process_device_raw(f.h, C.c_void_p(dev[b].data_ptr()), fmt, 2048.0, n, n, C.c_void_p(pcm.data_ptr()),
                                                  pcm.shape[1], C.byref(got), C.c_void_p(s_run.cuda_stream))
                    if rc != 0:
                        raise RuntimeError(L.fmx_last_error().decode())
                    ev_used[b].record(s_run)
                torch.cuda.synchronize()

            run(4)
            steps = 8
            t0 = time.perf_counter()
            run(steps)
            dt = time.perf_counter() - t0
            f.synchronize()
            bps = 2 if fmt == m.IQ_U8 else 8
            res[name] = {"channels": ch, "value": round(ch * n * steps / dt / 1e6, 3), "unit": "MS/s",
                         "pcie_GBps": round(ch * n * steps * bps / dt / 1e9, 2), "ms_per_step": round(dt / steps * 1e3, 3),
                         "realtime_channels_equiv": round(ch * n * steps / dt / 1e6 / 2.304, 1)}
            del f, host, dev, pcm
            torch.cuda.empty_cache()
        except Exception as e:                      # a leg must not take the headline line down
            res[name] = {"error": str(e)[:200]}
    res["what"] = ("pinned host IQ -> H2D copy on one stream, fmx_process_device_raw on another, two device buffers "
                   "(copy of step k+1 overlaps step k); PCIe-inclusive, never the headline value")
    return res


def host_call_leg(fmx_amd, local_rank):
    """host_call_latency in a process of its own -- what a receiver is: one handle, one stream, no other work on the device -- and, beside it,
    in this process, where the batch handles' streams and PyTorch's are alive (every copy and wait of the call then negotiates with them)."""
    here = host_call_latency(fmx_amd, local_rank)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-call-only"], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, LOCAL_RANK=str(local_rank)))
        res = json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:
        return dict(here, note="own-process run failed: %s" % str(e)[:120])
    if "error" not in res:
        res["process"] = "its own (one handle, nothing else on the device: the receiver's situation)"
        res["ms_median_inside_the_bench_process"] = here.get("ms_median")
    return res


def host_call_latency(fmx_amd, local_rank, calls=300):
    """The single-receiver drop-in: fmx_process_host with the reference's 16384-sample block (fm-processor.cpp:374),
    pageable numpy buffers as the Qt adapter hands them over.  Real time needs one call per 7.11 ms."""
    m = fmx_amd.fmx
    try:
        f = fmx_amd.Fmx(1, device=local_rank, max_block=16384)
        for pid, v in ((m.P_BANDWIDTH, 165000), (m.P_LF_CUTOFF, 15000), (m.P_DEEMPHASIS, 50), (m.P_VOLUME_DB, -6.0)):
            f.set_param(pid, v)
        rng = np.random.default_rng(1)
        iq = (rng.random((16384, 2), dtype=np.float32) - 0.5)
        for _ in range(20):
            f.process_host(iq)
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            f.process_host(iq)
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts) * 1e3
        return {"block": 16384, "calls": calls, "ms_median": round(float(np.median(ts)), 4), "ms_p99": round(float(np.percentile(ts, 99)), 4),
                "ms_mean": round(float(ts.mean()), 4), "MSps_one_channel": round(16384 / float(np.median(ts)) / 1e3, 2),
                "realtime_budget_ms": round(16384 / 2304.0, 3)}
    except Exception as e:
        return {"error": str(e)[:200]}


if __name__ == "__main__":
    main()
