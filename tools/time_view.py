"""view camera against the segmentation camera, one process on one GPU, HIP events:
sdx_render_segmentation (k_seg_camera: every pixel against all 171 boxes) and sdx_render_view (culled 16 x 16 tiles) on the same
BlockAssemblySearch sim, N envs, scene camera, 128 x 128 - the shape Search's reset renders at.  Both are warmed up, then alternated:
REPS repetitions of CALLS back-to-back calls each; median and spread (min, max) of the per-call time.  Also, without a bound:
COLLISION geometry with all three outputs at that shape, and one env at 512 x 512.
usage: python tools/time_view.py [N] [--json PATH]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd.sim import SdxSim  # noqa: E402

REPS, CALLS = 30, 8


def scattered(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(n, 72, 7)
    for e in range(n):
        p[e, :, 0] = 0.05 + 0.4 * torch.rand(72, generator=g)
        p[e, :, 1] = 0.02 + 0.34 * torch.rand(72, generator=g)
        p[e, :, 2] = 0.63 + 0.12 * torch.rand(72, generator=g)
        q = torch.randn(72, 4, generator=g)
        p[e, :, 3:7] = q / q.norm(dim=1, keepdim=True)
    return p


def main(argv):
    n = int(argv[0]) if argv and not argv[0].startswith("-") else 128
    path = argv[argv.index("--json") + 1] if "--json" in argv else ""
    s = SdxSim(n, device="cuda:0", seed=2, task_kind=3)
    s.ROOT.view(n, 142, 13)[:, 9:81, :7] = scattered(n).cuda()
    s.refresh_kinematics()
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = {}

    def view(key, ids_, size, geometry, **which):
        outs[key] = s.render_view(ids_, "scene", size, size, geometry, out=outs.get(key), **which)

    cases = {
        "segmentation_128": lambda: s.render_segmentation(),
        "view_bounds_label_128": lambda: view("a", ids, 128, "bounds", depth=False, label=True, rgb=False),
        "view_collision_all_128": lambda: view("b", ids, 128, "collision"),
        "view_collision_all_1env_512": lambda: view("c", one, 512, "collision"),
    }
    for f in cases.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0.record()
    for _ in range(REPS):
        for k, f in cases.items():                 # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / CALLS * 1e3)
    w1.record()
    torch.cuda.synchronize()
    window = w0.elapsed_time(w1) * 1e-3
    same = float((outs["a"]["label"].clamp(min=0) != s.SEG_IMAGE).float().mean())
    res = {"what": "tools/time_view.py: us per call (HIP events), %d repetitions of %d calls each, alternating, after warm-up; one MI355X" % (REPS, CALLS),
           "envs": n, "window_s": round(window, 3), "label_pixels_differing_from_segmentation_image": same}
    for k, v in times.items():
        res[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    res["view_bounds_over_segmentation"] = round(res["view_bounds_label_128"]["median_us"] / res["segmentation_128"]["median_us"], 4)
    print(json.dumps(res, indent=1))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
    s.close()
    assert window >= 0.2, window


if __name__ == "__main__":
    main(sys.argv[1:])
