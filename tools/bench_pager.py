"""Timing of the pager stage (mfm_pocsag_process_device / mfm_flex_process_device / mfm_ais_process_device) on
resident PCM: idle channels (sync search only), busy channels (back-to-back POCSAG batches / FLEX frames / AIS packets)
and a mix.  One JSON line per scenario.

    python tools/bench_pager.py [--proto pocsag|flex|ais] [--channels 64] [--samples 699050] [--iters 20]

(FLEX: 699 050 samples at 25 kS/s are 447 392 at 16 kHz.  AIS: one 2^26-sample block at 2.4 MS/s is 1 398 101 samples
at 48 kHz; --samples defaults to that for --proto ais.)

Used for DESIGN.md section 9 and profiles/r01_pager_*; not part of bench.py's contract line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--proto", default="pocsag", choices=["pocsag", "flex", "ais"])
    args = ap.parse_args()
    if not args.samples:
        args.samples = 1398101 if args.proto == "ais" else 699050
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    sy = pkg.synth
    C, n = args.channels, args.samples
    rng = np.random.RandomState(3)
    if args.proto == "flex":
        return flex_main(pkg, torch, C, n, args.iters, rng)
    if args.proto == "ais":
        return ais_main(pkg, torch, C, n, args.iters, rng)
    msgs = [(0x12345, 3, 2, sy.pocsag_alpha_words("THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG 0123456789 " * 3 + "\x04"))] * 12
    bits = sy.pocsag_bits(sy.pocsag_batches(msgs))
    burst = {b: sy.pocsag_pcm(bits, b, noise=900, lead=3000, trail=3000, seed=b) for b in (512, 1200, 2400)}

    def busy(baud, seed):
        x = np.concatenate([burst[baud]] * (n // burst[baud].size + 1))[:n].copy()
        return x

    idle = rng.normal(0, 1500, (C, n)).round().astype(np.int16)
    full = np.stack([busy((512, 1200, 2400)[c % 3], c) for c in range(C)])
    mix = idle.copy()
    mix[::4] = full[::4]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for name, host in (("idle", idle), ("busy", full), ("mixed", mix)):
        x = torch.from_numpy(host).to(dev)
        pg = pkg.Pocsag(C, n, device=0)
        for _ in range(3):
            pg.process_device(x.data_ptr(), n, n, stream=stream)
        nev = len(pg.fetch_events())
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.iters):
            pg.process_device(x.data_ptr(), n, n, stream=stream)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.iters
        print(json.dumps({"scenario": name, "channels": C, "pcm_samples_per_channel": n, "ms_per_block": round(ms, 4),
                          "pcm_msamples_per_s": round(C * n / ms / 1e3, 1), "events_last_block": nev,
                          "pcm_read_gbps": round(C * n * 2 / ms / 1e6, 1)}), flush=True)
        pg.close()


def flex_main(pkg, torch, C, n, iters, rng):
    sy = pkg.synth
    recs = [dict(kind="alnum", capcode=1000 + i, text="THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG %d" % i) for i in range(4)]
    frames = []
    for k in range(4):
        ph = {p: sy.flex_phase_words(recs) for p in sy.FLEX_CODINGS[k]["phases"]}
        frames.append(sy.flex_pcm([sy.flex_frame_levels(k, 1, k, ph)], noise=300, seed=k))
    idle = rng.normal(0, 1500, (C, n)).round().astype(np.int16)
    full = np.stack([np.concatenate([frames[c % 4]] * (n // 30000 + 2))[(c * 977) % 30000:][:n] for c in range(C)])
    mix = idle.copy()
    mix[::4] = full[::4]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for name, host in (("idle", idle), ("busy", full), ("mixed", mix)):
        x = torch.from_numpy(host).to(dev)
        fx = pkg.Flex(C, n, device=0)
        for _ in range(3):
            fx.process_device(x.data_ptr(), n, n, stream=stream)
        ev, fw = fx.fetch_events()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fx.process_device(x.data_ptr(), n, n, stream=stream)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / iters
        print(json.dumps({"proto": "flex", "scenario": name, "channels": C, "pcm_samples_per_channel": n,
                          "ms_per_block": round(ms, 4), "pcm_msamples_per_s": round(C * n / ms / 1e3, 1),
                          "events_last_block": int(len(ev)), "frames_last_block": int(len(fw)),
                          "pcm_read_gbps": round(C * n * 2 / ms / 1e6, 1)}), flush=True)
        fx.close()


HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E, as bench.py


def ais_main(pkg, torch, C, n, iters, rng):
    """idle: noise only; busy: packets of types 1, 4, 5 back to back (one flag apart); mixed: every fourth channel
    busy.  Bytes read = the PCM once (2 bytes per sample), what the slicer must read; the bit planes the later kernels
    read and write are 1/8 and 2/8 of a byte per sample on top."""
    sy = pkg.synth
    pl = [sy.ais_type1(123456789, lon=-7234567, lat=2345678), sy.ais_type4(111222333),
          sy.ais_type5(987654321, callsign="TEST", ship_name="BENCH", destination="HBM")]
    train = sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(pl[k % 3]) for k in range(30)], gap_bits=0), noise=400, seed=1)
    idle = rng.normal(0, 1500, (C, n)).round().astype(np.int16)
    full = np.stack([np.concatenate([train] * (n // train.size + 2))[(c * 977) % train.size:][:n] for c in range(C)])
    mix = idle.copy()
    mix[::4] = full[::4]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for name, host in (("idle", idle), ("busy", full), ("mixed", mix)):
        x = torch.from_numpy(host).to(dev)
        st = pkg.Ais(C, n, device=0)
        for _ in range(3):
            st.process_device(x.data_ptr(), n, n, stream=stream)
        ev = st.fetch_events()
        torch.cuda.synchronize()
        reps = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                st.process_device(x.data_ptr(), n, n, stream=stream)
            t1.record()
            torch.cuda.synchronize()
            reps.append(t0.elapsed_time(t1) / iters)
        ms = float(np.median(reps))
        read = C * n * 2
        print(json.dumps({"proto": "ais", "scenario": name, "channels": C, "pcm_samples_per_channel": n,
                          "ms_per_block": round(ms, 4), "ms_reps": [round(r, 4) for r in reps],
                          "pcm_msamples_per_s": round(C * n / ms / 1e3, 1), "events_last_block": int(len(ev)),
                          "valid_packets_last_block": int(ev["fcs_valid"].sum()), "pcm_bytes_read": read,
                          "pcm_read_gbps": round(read / ms / 1e6, 1),
                          "frac_hbm_peak": round(read / ms / 1e6 / HBM_PEAK_GBPS, 3),
                          "realtime_factor": round(n / 48000.0 / (ms * 1e-3), 1)}), flush=True)
        st.close()


if __name__ == "__main__":
    main()
