"""Per-wave timing of the fast SP forward's decoder-matrix (C1 / C2) ingest.

tools/phase_stamps.py stamps the example workgroup's phases from thread 0.  This tool answers
what those cannot: when each WAVE's last C register lands, when the W rows land on waves 0-3,
when the A-row DMAs land on waves 4-7 and when P is published -- from s_memrealtime stamps
(100 MHz) each wave takes into registers where it waits anyway and stores at the end of the
kernel (rae_sp.hpp, -DRAE_WSTAMPS: 8 u64 per wave into a buffer of their own, handed over by
rae_debug_wave_stamps; without it such a library writes no wave stamps).

    python tools/c_stream_stamps.py [--config c3] [--iters 10] [--batch-size 100]
    RAE_VARIANT="-DRAE_FWD_CE47=0" python tools/c_stream_stamps.py     # another split

Slots (us from the workgroup's first wave entry, median / max over workgroups and launches):
  entry      the wave starts
  early      waves 4-7: the early tranche of C is issued; waves 0-3: the descriptor has landed
  issued     every load of the wave is issued
  W/A        waves 0-3: the W rows have landed (partial sums stored);
             waves 4-7: the A-row DMAs, Ab and the early tranche have landed
  C          the wave's last C register has landed (not taken on wave 0, which runs the chain)
  P          wave 0: P published; other waves: P seen
  C.P        the wave's share of C.P is done
  end        the wave ends
Waves 1-7 only poll the P flag between `issued` and `P`, so the waits behind `W/A` and `C`
cost the chain nothing; wave 0 takes no wait it would not take anyway.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "relation-autoencoder_amd")
VARIANT = os.environ.get("RAE_VARIANT", "")      # extra -D flags: a diagnostic A/B build
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
NW, NS = 8, 8                                    # waves per workgroup, slots per wave
SLOTS = ["entry", "early", "issued", "W/A", "C", "P", "C.P", "end"]


def build_diag():
    import __graft_entry__ as ge
    tag = ("_" + VARIANT.replace("-D", "").replace("=", "").replace(" ", "_")) if VARIANT else ""
    out = os.path.join(PKG, "rae", f"librae_hip_wstamps{tag}.so")
    src = os.path.join(PKG, "csrc", "rae.hip")
    _lib = ge._lib_mod()
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in _lib.source_files()):
        subprocess.run([ge.HIPCC, *_lib.BUILD_FLAGS, "-DRAE_STAMPS", "-DRAE_DIAG", "-DRAE_WSTAMPS",
                        *VARIANT.split(), src, "-o", out], check=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=100)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    lib_path = build_diag()
    if args.build_only:
        print(lib_path)
        return
    os.environ["RAE_LIB"] = lib_path
    import torch
    import bench
    from rae import _lib
    from rae.data import synthetic_dataset
    from rae.inducer import ReconstructInducer
    lib = _lib.load()
    lib.rae_debug_wave_stamps.argtypes = [C.c_void_p, C.c_void_p]
    lib.rae_debug_grid.argtypes = [C.c_void_p, C.c_void_p]
    cfg = bench.CONFIGS[args.config]
    dev = torch.device("cuda", 0)
    data, gold = synthetic_dataset(cfg["N"], cfg["d"], cfg["ntrue"], seed=1234)
    ind = ReconstructInducer(data, gold, np.random.RandomState(2), 1, 0.1, args.batch_size,
                             cfg["r"], cfg["m"], cfg["s"], 0.0, 0.0, "adagrad", "stamps",
                             cfg["dec"], False, True, False, 1.0, device=dev, graph_chunk=1)
    ind.compile_function()
    eng = ind.engine
    n1, n2 = ind.draw_epoch_negatives()
    eng.set_epoch_negatives(n1, n2)
    eng.run(0, 20, graph=False)
    torch.cuda.synchronize()
    grid = (C.c_int * 4)()
    lib.rae_debug_grid(eng.plan, grid)
    gf = grid[0]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.rae_build_index(eng.plan, 20, args.iters, st)
    per = []
    for it in range(args.iters):
        buf = torch.zeros(gf * NW * NS, dtype=torch.int64, device=dev)
        lib.rae_debug_wave_stamps(eng.plan, C.c_void_p(buf.data_ptr()))
        lib.rae_step_forward_at(eng.plan, 20 + it, st)
        torch.cuda.synchronize()
        lib.rae_debug_wave_stamps(eng.plan, None)
        lib.rae_step_update_at(eng.plan, 20 + it, st)
        torch.cuda.synchronize()
        wv = buf.cpu().numpy().reshape(gf, NW, NS).astype(np.float64) / 100.0   # -> us
        ok = wv[:, :, 7].min(axis=1) > 0          # general-path rows store no wave stamps
        wv = wv[ok]
        t0 = wv[:, :, 0].min(axis=1)[:, None, None]
        per.append(np.where(wv > 0, wv - t0, np.nan))
    per = np.concatenate(per)
    print(f"config {args.config} variant '{VARIANT}': {per.shape[0]} workgroup samples "
          f"({args.iters} launches of {gf}); us from the workgroup's first wave entry, median/max")
    print("  wave  " + "  ".join(f"{s:>11s}" for s in SLOTS))
    for w in range(NW):
        cells = []
        for k in range(NS):
            col = per[:, w, k]
            col = col[~np.isnan(col)]
            cells.append(f"{np.median(col):5.2f}/{col.max():5.2f}" if col.size else "     -     ")
        print(f"  {w:4d}  " + "  ".join(cells))
    lastC = np.nanmax(per[:, 1:, 4], axis=1)
    p_pub = per[:, 0, 5]
    print(f"  last C register of waves 1-7 lands: median {np.median(lastC):.2f} max {lastC.max():.2f}; "
          f"P published: median {np.median(p_pub):.2f} max {p_pub.max():.2f}; "
          f"C behind P in {100.0 * np.mean(lastC > p_pub):.0f} % of workgroups, by median "
          f"{np.median(lastC - p_pub):.2f} us")
    end = np.nanmax(per[:, :, 7], axis=1)
    print(f"  workgroup end: median {np.median(end):.2f} max {end.max():.2f}")


if __name__ == "__main__":
    main()
