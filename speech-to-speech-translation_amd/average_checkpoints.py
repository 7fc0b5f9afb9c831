"""``average_checkpoints``: stage 6 of the recipes (run_baseline.sh), the counterpart of ``scripts/average_checkpoints.py``
followed by ``examples/s2s_trans/convert_pt_to512.py``.

    python -m s2st_amd.average_checkpoints --inputs CKPT_DIR --num-epoch-checkpoints 15 \
        --output CKPT_DIR/checkpoint_last_avg15.pt [--decoder-embed-dim 512]

Every inference stage of the recipe reads the averaged file.  Rules of the reference's script, restated:

* ``--num-epoch-checkpoints n`` / ``--num-update-checkpoints n``: ``--inputs`` names ONE directory; the files matching
  ``checkpoint(\\d+)\\.pt`` / ``checkpoint_\\d+_(\\d+)\\.pt`` are ordered by that number, ``--checkpoint-upper-bound`` drops the
  larger ones, the newest ``n`` are averaged; fewer than ``n`` is an error.  Without either flag ``--inputs`` lists the files.
* the model key lists of all files must be equal, in order (``KeyError`` otherwise);
* half tensors are summed in fp32; the sum of a floating tensor is divided by ``n``, an integer tensor
  (``num_batches_tracked``) is floor-divided (``//=``);
* everything but ``model`` -- cfg, optimizer state, histories -- is the first listed file's.

``--decoder-embed-dim N`` sets ``cfg["model"].decoder_embed_dim`` of the output: the one line of convert_pt_to512.py.
The output is in the reference's ``.pt`` layout and loads through ``generate_waveform`` / ``generate_text`` here.
"""
from __future__ import annotations

import argparse
import collections
import os
import re
import sys
from typing import Any, Dict, List, Optional

import torch

from . import checkpoint_utils

EPOCH_RE = re.compile(r"checkpoint(\d+)\.pt")
UPDATE_RE = re.compile(r"checkpoint_\d+_(\d+)\.pt")


def last_n_checkpoints(paths: List[str], n: int, update_based: bool, upper_bound: Optional[int] = None) -> List[str]:
    if len(paths) != 1:
        raise ValueError("with --num-epoch-checkpoints / --num-update-checkpoints, --inputs names one directory")
    rx = UPDATE_RE if update_based else EPOCH_RE
    entries = []
    for f in os.listdir(paths[0]):
        m = rx.fullmatch(f)
        if m is not None and (upper_bound is None or int(m.group(1)) <= upper_bound):
            entries.append((int(m.group(1)), f))
    if len(entries) < n:
        raise RuntimeError(f"found {len(entries)} checkpoint files but need at least {n}")
    return [os.path.join(paths[0], f) for _, f in sorted(entries, reverse=True)[:n]]


def average_checkpoints(inputs: List[str]) -> Dict[str, Any]:
    sums: "collections.OrderedDict[str, torch.Tensor]" = collections.OrderedDict()
    keys = new_state = None
    for path in inputs:
        state = checkpoint_utils.load_checkpoint_to_cpu(path)
        if new_state is None:
            new_state = state  # the settings of the first file
        model = state["model"]
        if keys is None:
            keys = list(model.keys())
        elif keys != list(model.keys()):
            raise KeyError(f"for checkpoint {path}, expected list of params: {keys}, but found: {list(model.keys())}")
        for k in keys:
            p = model[k]
            if p.dtype == torch.float16:
                p = p.float()
            if k not in sums:
                sums[k] = p.clone()  # (a parameter may be shared between two names)
            else:
                sums[k] += p
    n = len(inputs)
    for v in sums.values():
        if v.is_floating_point():
            v.div_(n)
        else:
            v //= n
    new_state["model"] = sums
    return new_state


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="s2st_amd.average_checkpoints",
                                description="average the parameters of checkpoints into a new checkpoint")
    p.add_argument("--inputs", required=True, nargs="+", help="checkpoint files, or one directory with --num-*-checkpoints")
    p.add_argument("--output", required=True, metavar="FILE")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--num-epoch-checkpoints", type=int, help="average the last n checkpoint<epoch>.pt of the directory")
    g.add_argument("--num-update-checkpoints", type=int, help="average the last n checkpoint_<epoch>_<update>.pt")
    p.add_argument("--checkpoint-upper-bound", type=int, help="the largest epoch / update number to use")
    p.add_argument("--decoder-embed-dim", type=int, default=None,
                   help="set cfg['model'].decoder_embed_dim of the output (examples/s2s_trans/convert_pt_to512.py)")
    return p


def main(argv: Optional[List[str]] = None) -> Dict[str, Any]:
    args = make_parser().parse_args(argv)
    num = args.num_update_checkpoints if args.num_update_checkpoints is not None else args.num_epoch_checkpoints
    if args.checkpoint_upper_bound is not None and num is None:
        raise SystemExit("--checkpoint-upper-bound requires --num-epoch-checkpoints or --num-update-checkpoints")
    inputs = list(args.inputs)
    if num is not None:
        inputs = last_n_checkpoints(inputs, num, args.num_update_checkpoints is not None, args.checkpoint_upper_bound)
        print("averaging checkpoints: ", inputs)
    state = average_checkpoints(inputs)
    if args.decoder_embed_dim is not None:
        m = state["cfg"]["model"]
        if isinstance(m, dict):
            m["decoder_embed_dim"] = args.decoder_embed_dim
        else:
            m.decoder_embed_dim = args.decoder_embed_dim
    tmp = args.output + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, args.output)
    print(f"Finished writing averaged checkpoint to {args.output}")
    return state


if __name__ == "__main__":
    main(sys.argv[1:])
