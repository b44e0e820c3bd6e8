"""Binding-site finder cost (dbfr_find_sites) next to the sampling of 40 poses per site found.

    python tools/sites_bench.py [--reps 5] [--steps 20] [--n 2000] [--out profiles/r11_sites_bench.json]

Writes one JSON object (and prints it).  Receptors: the six of tests/golden/sites_receptors.npz.  Legs:
  3dbs        3DBS alone (542 724 grid points, one launch);
  six         the six receptors in one call;
  tiled       the six tiled to --n receptors (config 4's target-fishing scale; several launches of <= 2^23 points).
For each: call_ms = HIP events around the dbfr_find_sites calls of the leg (device time of the kernels plus the gaps of the two
read-backs each call makes), and find_sites_wall_ms = wall clock of sites.find_sites (host bounds, staging, every launch, copy
back, Site building), synchronised; medians of --reps after one warm-up.  The sampling time is measured on one 640-pose batch
of synthetic config 4 (16 complexes x 40 poses, --steps denoise steps, seeded random weights), scaled per pose to 40 poses per
site found; *_over_sample are the ratios.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchkit  # noqa: E402
from diffbindfr_amd import lib as L, posecheck, sites  # noqa: E402
import sites_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--n", type=int, default=2000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_sites_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")


def stage(recs):
    aa = torch.as_tensor(np.concatenate([r["aatype"] for r in recs])).to(dev)
    pos = torch.as_tensor(np.concatenate([r["pos"] for r in recs])).to(dev)
    msk = torch.as_tensor(np.concatenate([r["mask"] for r in recs])).to(dev)
    rp = np.concatenate([[0], np.cumsum([len(r["aatype"]) for r in recs])])
    return aa, pos, msk, rp


def library_calls(aa, pos, msk, rp):
    """The dbfr_find_sites calls find_sites makes for this batch, staged once: returns a function issuing them."""
    lib = L.load()
    o = sites.check_opts()
    S = o["max_sites"]
    mn, mx = sites._bounds(pos, msk, rp)
    npts = [int(np.prod(sites.grid_of(mn[p], mx[p], o["spacing"])[1])) for p in range(len(rp) - 1)]
    chunks, s = [], 0
    while s < len(npts):
        e, t = s + 1, npts[s]
        while e < len(npts) and t + npts[e] <= sites.LAUNCH_POINTS:
            t += npts[e]
            e += 1
        chunks.append((s, e, t))
        s = e
    cap = max(t for _, _, t in chunks)
    nb = C.c_size_t()
    L.check(lib.dbfr_sites_workspace_bytes(C.byref(L.SitesIn(n_prot=max(e - s for s, e, _ in chunks), n_res=len(aa), max_points=cap)),
                                           C.byref(nb)))
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
    rad = torch.as_tensor(posecheck.receptor_radius_table(), device=dev).contiguous()
    aa32 = aa.int().contiguous()
    opts = sites._c_opts(o)
    calls, keep = [], [ws, rad, aa32]
    for s, e, t in chunks:
        r0, r1, P = int(rp[s]), int(rp[e]), e - s
        sub = torch.as_tensor(rp[s:e + 1] - r0, dtype=torch.int32, device=dev)
        outs = [torch.empty(P, dtype=torch.int32, device=dev)] + [torch.empty(P * S, dtype=torch.int32, device=dev) for _ in range(3)] + \
               [torch.empty(P * S * 3, dtype=torch.int64, device=dev), torch.empty(P * S * 3, dtype=torch.float64, device=dev),
                torch.empty((r1 - r0) * S, dtype=torch.uint8, device=dev)]
        keep += [sub] + outs
        p = lambda x: C.c_void_p(x.data_ptr())
        cin = L.SitesIn(P, r1 - r0, t, p(sub), p(aa32[r0:r1]), p(pos[r0:r1]), p(msk[r0:r1]), p(rad))
        cout = L.SitesOut(*[p(x) for x in outs])
        calls.append((cin, cout))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(_keep=keep):
        for cin, cout in calls:
            L.check(lib.dbfr_find_sites(C.byref(cin), C.byref(opts), C.byref(cout), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), stream))
    return run, len(chunks), sum(npts)


recs = sites_ref.load_receptors(os.path.join(ROOT, "tests", "golden", "sites_receptors.npz"))
legs = {"3dbs": recs[:1], "six": recs, "tiled": [recs[k % 6] for k in range(args.n)]}
res = {"what": "binding-site detection (dbfr_find_sites) next to sampling 40 poses per site found",
       "device": torch.cuda.get_device_name(0)}
per_pose = benchkit.sample_seconds_per_pose(4, args.steps, args.reps, dev)
for name, rr in legs.items():
    aa, pos, msk, rp = stage(rr)
    run, n_launch, n_points = library_calls(aa, pos, msk, rp)
    t_call = benchkit.events(run, args.reps)[0]
    found = []
    t_wall = benchkit.wall(lambda: found.__setitem__(slice(None), sites.find_sites(aa, pos, msk, res_ptr=rp)), args.reps)
    n_sites = sum(len(x) for x in found)
    sample_s = per_pose * 40 * n_sites
    res[name] = {"receptors": len(rr), "grid_points": int(n_points), "launches": n_launch, "sites_kept": n_sites,
                 "call_ms": round(t_call * 1e3, 3), "find_sites_wall_ms": round(t_wall * 1e3, 2),
                 "sample_s_scaled": round(sample_s, 3), "call_over_sample": round(t_call / sample_s, 7),
                 "find_sites_over_sample": round(t_wall / sample_s, 7)}
    del aa, pos, msk
    torch.cuda.empty_cache()
res["sample_s_per_pose_cfg4"] = round(per_pose, 6)
res["timing"] = (f"call: HIP events around the dbfr_find_sites calls of the leg (kernels plus the read-back gaps), median of "
                 f"{args.reps} after one warm-up; find_sites: wall clock, synchronised, median of {args.reps}; sampling: {args.steps} "
                 f"steps of a 640-pose batch of synthetic config 4, per pose, scaled to 40 poses per site kept")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
benchkit.emit(res, args.out)
