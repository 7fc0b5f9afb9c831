#!/usr/bin/env python
"""Write tests/golden/ckpt_avg.npz: the reference's own scripts/average_checkpoints.py run on the three checkpoints of
tests/ckpt_avg_fixture.py, in the order newest first (what its --num-epoch-checkpoints 3 selects).  Needs the reference
tree (a build container only); the fixture holds numbers, no program text.

    python tools/gen_golden_ckpt_avg.py REFERENCE_ROOT
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))
for _n, _t in dict(float=float, int=int, bool=bool, object=object, complex=complex, str=str).items():
    if not hasattr(np, _n):  # (the reference predates numpy 1.24)
        setattr(np, _n, _t)

from ckpt_avg_fixture import make_inputs  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("ref_average_checkpoints", os.path.join(REF, "scripts", "average_checkpoints.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    with tempfile.TemporaryDirectory() as d:
        make_inputs(os.path.join(ROOT, "tests", "golden"), d)
        inputs = ref.last_n_checkpoints([d], 3, False)
        import argparse
        import torch
        with torch.serialization.safe_globals([argparse.Namespace]):  # (the reference predates torch.load's weights_only default)
            state = ref.average_checkpoints(inputs)
    out = {"order": np.asarray([os.path.basename(p) for p in inputs]),
           "which_file": np.asarray(state["extra_state"]["which_file"])}
    for k, v in state["model"].items():
        out["model." + k] = v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "ckpt_avg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
