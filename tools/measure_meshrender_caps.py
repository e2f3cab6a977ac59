#!/usr/bin/env python
"""Measures how far a view of the baked mesh is from the neural view it was baked from, WITHOUT the new kernels: the float64 path of
tests/meshrender_restatement.py (rasteriser and G-buffer in double precision on the CPU) on the end-to-end scene of
tests/meshrender_scene.py, shaded by the same existing sg_render call.  The maxima over the interior pixels go to
tests/golden/meshrender_caps.json; tests/test_meshrender_gpu.py holds the kernels' view to twice these (DESIGN 6's convention for caps
that cannot be derived).  Needs the GPU (the neural forward, the bake and the shading run there).

    python tools/measure_meshrender_caps.py [--out tests/golden/meshrender_caps.json]
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import meshrender_scene as ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "meshrender_caps.json"))
    a = ap.parse_args(argv)
    with torch.no_grad():
        scene = ms.build(torch.device("cuda:0"))
        neural_mask = scene["neural"]["network_object_mask"].reshape(ms.H, ms.W).cpu().numpy()
        inner = ms.interior(neural_mask)
        view = ms.float64_view(scene, vis="network")
        caps = ms.distances(view, scene["neural"], inner)
    differ = view["network_object_mask"].reshape(ms.H, ms.W) != neural_mask
    doc = {"command": "python tools/measure_meshrender_caps.py", "date": datetime.date.today().isoformat(),
           "what": "max |float64 mesh view - neural forward('Material')| over the interior pixels of the neural hit mask; "
                   "the test's cap is 2 x these",
           "scene": {"seed": 0, "mesh_resolution": ms.MESH_RESOLUTION, "refine": ms.REFINE, "atlas_resolution": ms.ATLAS_RESOLUTION,
                     "size": ms.H, "vis": "network", "filter": 1, "faces": int(scene["mesh"].faces.shape[0])},
           "interior_pixels": int(inner.sum()), "hit_pixels": int(neural_mask.sum()),
           "mask_differences": int(differ.sum()), "mask_differences_off_boundary": int((differ & ~ms.boundary(neural_mask)).sum()),
           "caps": caps}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
