"""``segment``: cut long recordings at their pauses.

    python -m s2st_amd.segment AUDIO... --results-path OUT [--max-segment-s 30] [--min-segment-s 1] [--silence-db 40] \
        [--cut-penalty-db 40] [--segment-pad-ms 100] [--segmenter device|host] [--write-wavs]

What ``translate --segment long`` does in front of the model, on its own (cutting a corpus, say): ``OUT/segments.tsv`` holds one
row per segment,

    id  k  src_start_s  src_end_s  trim_start_s  trim_end_s  dropped

(``id``: the file's stem; the ``src`` spans of a recording tile it without gaps; a ``dropped`` segment holds no speech frame),
and with ``--write-wavs`` the trimmed span of every segment that is not dropped becomes ``OUT/wav/<id>#<k>.wav`` (16-bit PCM;
float input rounded by the ``s2st_wave_to_pcm16`` rule).  The definition is ``segmentation``'s (exact integers, ties to the
fewest and latest cuts); ``--segmenter device`` (csrc/segment.hip) and ``--segmenter host`` (numpy) write the same bytes.
**Parity unpinned: the reference has no segmentation.**  Recordings are segmented at their own rate, all files of one rate
in one call.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from typing import Dict, List, Optional

import torch

from . import segmentation as sgm
from .data.audio_utils import read_audio
from .inference_common import default_device, write_pcm16


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="s2st_amd.segment", allow_abbrev=False)
    p.add_argument("audio", nargs="+", help="audio files; ids are the file stems")
    p.add_argument("--results-path", required=True)
    sgm.add_segment_flags(p)
    p.set_defaults(max_segment_s=30.0)  # (no model here: the limit of every recipe, 3000 frames)
    p.add_argument("--write-wavs", action="store_true", help="also write the trimmed segments as OUT/wav/<id>#<k>.wav")
    return p


def main(argv: Optional[List[str]] = None, device: Optional[torch.device] = None) -> Dict:
    args = make_parser().parse_args(argv)
    opt = sgm.segment_frames(args, None)
    ids = [Path(f).stem for f in args.audio]
    if len(set(ids)) != len(ids):
        raise SystemExit(f"segment: duplicate ids {sorted({i for i in ids if ids.count(i) > 1})}")
    if args.segmenter == "device" and device is None:
        device = default_device("segment", needed_for="--segmenter device", without="--segmenter host")
    audio = [read_audio(f) for f in args.audio]
    segs: List = [None] * len(audio)
    for rate in sorted({r for _, r in audio}):
        idx = [i for i, (_, r) in enumerate(audio) if r == rate]
        pcm = [sgm.host_pcm16(audio[i][0]) for i in idx]
        for i, s in zip(idx, sgm.segment(pcm, rate, opt["min_len"], opt["max_len"], sgm.SMOOTH_FRAMES, opt["silence_db"],
                                         opt["cut_penalty_db"], opt["pad"], device=device, segmenter=args.segmenter)):
            segs[i] = s
    out_root = Path(args.results_path)
    out_root.mkdir(exist_ok=True, parents=True)
    written = [str(out_root / "segments.tsv")]
    sgm.write_segments_tsv(written[0], [r for i, s in zip(ids, segs) for r in sgm.segment_rows(i, s)])
    if args.write_wavs:
        (out_root / "wav").mkdir(exist_ok=True)
        for i, (w, rate), s in zip(ids, audio, segs):
            pcm = sgm.host_pcm16(w)
            for k in range(len(s)):
                if not s.dropped[k]:
                    a, b = (int(v) for v in s.trim_samples[k])
                    written.append(str(out_root / "wav" / f"{i}#{k}.wav"))
                    write_pcm16(written[-1], pcm[a:b], rate)
    return {"recordings": len(audio), "segments": sum(len(s) for s in segs),
            "dropped": sum(int(s.dropped.sum()) for s in segs), "files": written}


def cli_main():
    r = main(sys.argv[1:])
    print(f"cut {r['recordings']} recordings into {r['segments']} segments ({r['dropped']} without speech); "
          f"{len(r['files'])} files under the results path")


if __name__ == "__main__":
    cli_main()
