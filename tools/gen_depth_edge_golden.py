"""Write tests/golden/depth_edge_cases.safetensors + .json: what the REFERENCE's depth_edge (modeling/pi3/utils/geometry.py)
answers on the depth maps of tests/cloud_check.py::edge_cases, for every (atol, rtol) pair of cloud_check.EDGE_TOLS.

TEST INFRASTRUCTURE.  Runs where the reference tree is checked out (CPU only, never on the GPU box): the reference file is
imported by path and only called.  tests/test_cloud_cpu.py compares cloud_check.edge_mask - the rule csrc/cloud.hip implements -
with the masks stored here, bit for bit.

    python tools/gen_depth_edge_golden.py [--reference DIR]

Layout: per case `d_HxW` fp32 [3, H, W] (the depths, so that the fixture does not depend on numpy's generator) and `e_HxW` uint8
[3, H, W] whose bit i is the reference's edge mask under EDGE_TOLS[i]; the JSON names the pairs and the shapes."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_depth_edge(reference_root):
    path = os.path.join(reference_root, "modeling", "pi3", "utils", "geometry.py")
    spec = importlib.util.spec_from_file_location("_reference_pi3_geometry", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.depth_edge


def reference_bits(depth_edge, depth, tols):
    """uint8 [N,H,W]: bit i = depth_edge(depth, *tols[i])"""
    bits = np.zeros(depth.shape, dtype=np.uint8)
    for i, (atol, rtol) in enumerate(tols):
        e = depth_edge(torch.from_numpy(depth.copy()), atol=atol, rtol=rtol)
        bits |= e.numpy().astype(np.uint8) << i
    return bits


def main(argv=None):
    import cloud_check
    from oracle.ref_shim import REF_ROOT
    from safetensors.numpy import save_file
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REF_ROOT)
    args = ap.parse_args(argv)
    depth_edge = load_depth_edge(args.reference)
    tensors = {}
    for name, d in cloud_check.edge_cases().items():
        tensors[name] = d
        tensors["e" + name[1:]] = reference_bits(depth_edge, d, cloud_check.EDGE_TOLS)
    save_file(tensors, cloud_check.GOLDEN + ".safetensors")
    json.dump(dict(tols=[list(t) for t in cloud_check.EDGE_TOLS], views=cloud_check.EDGE_N,
                   shapes=[list(s) for s in cloud_check.EDGE_SHAPES],
                   source="reference modeling/pi3/utils/geometry.py::depth_edge, kernel_size 3, mask None, torch CPU"),
              open(cloud_check.GOLDEN + ".json", "w"), indent=1)
    print(cloud_check.GOLDEN + ".safetensors", os.path.getsize(cloud_check.GOLDEN + ".safetensors"), "bytes")


if __name__ == "__main__":
    main()
