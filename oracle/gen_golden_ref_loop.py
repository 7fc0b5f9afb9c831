#!/usr/bin/env python3
"""Golden of the REFERENCE's own training loop on the NANO model (build container only):
    python oracle/gen_golden_ref_loop.py      # writes tests/golden/ref_loop.npz
TEST INFRASTRUCTURE.  The reference's S2STTransformerModel + Tacotron2Criterion (oracle/gen_golden.py build_reference, the
synthetic weights of seed 0) driven by fairseq's own step -- FairseqTask.train_step + FairseqAdam + clip_grad_norm_ in the
order of fairseq/trainer.py:760-905 (tests/ref_loop_child.py `drive`) -- for three updates with update-freq 1 and 2 on the
NANO batches: losses, gradient norms and logging outputs.  Of the parameters after the last update only two numbers per
tensor are stored: max |p_ref| and max |p_ref - p_oracle|, p_oracle being the oracle model (oracle/s2st_oracle.py) after the
same updates under the restated step (tests/ref_loop_child.py `oracle_loop`).  tests/test_reference_loop.py recomputes
p_oracle, so that  max |p_ours - p_oracle| + max |p_ref - p_oracle|  bounds  max |p_ours - p_ref|  element by element."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ref_loop_child as RL  # noqa: E402


def main():
    driver = RL.fairseq_driver()
    if driver is None:
        raise SystemExit("needs the reference tree (fairseq) on the import path")
    import gen_golden as GG
    from synth_weights import load_synth
    from test_engine import NANO
    out = {}
    for uf in (1, 2):
        _, model, crit = GG.build_reference(NANO)
        load_synth(model, 0)
        losses, gnorms, logs, pa = RL.drive(driver, None, model, crit, RL.loop_batches(), uf)
        po = RL.oracle_loop(uf)
        assert sorted(po) == sorted(pa), "the oracle's parameter names differ from the reference's"
        g = f"uf{uf}."
        out[g + "loss"] = np.asarray(losses, np.float64)
        out[g + "gnorm"] = np.asarray(gnorms, np.float64)
        for k in RL.LOG_KEYS:
            out[g + "log." + k] = np.asarray([lg[k] for lg in logs], np.float64)
        worst = 0.0
        for n, p in pa.items():
            pmax, pdev = float(p.abs().max()), float((p - po[n]).abs().max())
            out[g + "pmax." + n] = np.float64(pmax)
            out[g + "pdev." + n] = np.float64(pdev)
            worst = max(worst, pdev / (pmax + 1e-6))
        print(f"update-freq {uf}: oracle vs reference parameters, worst max|diff| / max|p| = {worst:.3g}")
    path = os.path.join(ROOT, "tests", "golden", "ref_loop.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
