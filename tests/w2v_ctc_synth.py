"""wav2vec 2.0 CTC test geometries, seeded synthetic weights and audio, and a float64 restatement of the forward.

Shared by tests/test_asr_bleu.py and tools/gen_golden_w2v_ctc.py (which runs ``transformers.Wav2Vec2ForCTC`` on what this
module makes and writes tests/golden/w2v_ctc.npz).

Weight recipe (documented, CPU, deterministic): the tensors the forward reads are enumerated in ``state_dict_shapes`` order
under the library's names (the positional convolution's weight norm as ``weight_g`` / ``weight_v``); tensor number i is
drawn from ``torch.Generator().manual_seed(SEED0 + i)``: matrices and convolutions ``N(0, 1 / fan_in)`` (convolutions
``2 / fan_in``: a GELU halves the power), LayerNorm weights ``1 + 0.1 N(0, 1)``, biases ``0.1 N(0, 1)``, ``weight_g ~
U(0.5, 1.5) sqrt(embed / taps)`` (so g != ||v||: the fold is exercised), the transformer branches' output matrices scaled by
``BRANCH_SCALE``, ``lm_head`` by ``LM_SCALE`` with ``LM_BLANK_BIAS`` added to the blank's bias (so that blanks and repeats
occur and the collapse has work to do).

Two heads per geometry replace ``synth_state``'s own ``lm_head`` wherever a golden is involved (``with_head``).  Both
were picked, by seed, so that the word delimiter ``|`` is emitted inside a transcript, at an utterance's start or end and
twice in a row around a blank: the id -> text mapping (delimiter -> space, strip) is compared with the library's.  The
"rich" head (``rich_head``) gives transcripts over the whole alphabet, but 32 equally scaled random rows
put the two best logits of most frames closer together than bf16 operands can resolve: the library's own
``torch.autocast(bfloat16)`` run moves the logits by ~4 % of their range (the seven conv + LayerNorm layers alone
contribute 1.6 % rms), and the gap between the two largest of 32 like-scaled values is below four times that in two frames
out of three, whatever ``LM_SCALE`` is (gap and error scale together).  The "peaked" head (``peaked_head``) is what the
fast-mode token check runs on: rows scaled geometrically (``rho ** rank`` over a seeded ranking of the 27 letters, the word
delimiter at a chosen rank), the special tokens' rows zero with bias -6, and a blank bias, i.e. a blank-dominated output with a few letters in play, as a
trained CTC model's; its (seed, rho, blank bias) per geometry were chosen so that at most 10 % of the frames have a top-1 /
top-2 margin within twice the fast-mode bound, which tools/gen_golden_w2v_ctc.py asserts.

The restatement is written from the architecture: (x - mean) / sqrt(var + 1e-7) over the utterance; seven times
Conv1d(bias) -> LayerNorm over channels -> GELU; LayerNorm -> Linear; x += GELU(pos_conv(x)) with the weight-normed grouped
convolution, padding k // 2 and the last frame dropped for even k; pre-LN layers x += attn(LN(x)), x += fc2(GELU(fc1(LN
(x)))); LayerNorm; lm_head.  One utterance at a time in float64: at an utterance's valid frames a padded batch with an
attention mask computes the same thing.
"""
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

SEED0 = 9000
BRANCH_SCALE = 0.5
LM_SCALE = 3.0
LM_BLANK_BIAS = 2.0

VOCAB = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4, "E": 5, "T": 6, "A": 7, "O": 8, "N": 9, "I": 10, "H": 11,
         "S": 12, "R": 13, "D": 14, "L": 15, "U": 16, "M": 17, "W": 18, "C": 19, "F": 20, "G": 21, "Y": 22, "P": 23, "B": 24,
         "V": 25, "K": 26, "'": 27, "X": 28, "J": 29, "Q": 30, "Z": 31}

_KS = [(10, 5)] + [(3, 2)] * 4 + [(2, 2)] * 2
TINY = {"conv": [(32, k, s) for k, s in _KS], "embed": 64, "layers": 3, "heads": 4, "ffn": 128, "conv_pos": 16,
        "conv_pos_groups": 4, "vocab": 32}
LARGE = {"conv": [(512, k, s) for k, s in _KS], "embed": 1024, "layers": 24, "heads": 16, "ffn": 4096, "conv_pos": 128,
         "conv_pos_groups": 16, "vocab": 32}
CONFIGS = {"tiny": TINY, "large": LARGE}
# ragged utterances per geometry: (samples, audio seed); tiny includes the shortest possible one (400 samples: 1 frame)
UTTS = {"tiny": [(5000, 11), (400, 12), (12345, 13), (8000, 14)], "large": [(16000, 21), (9000, 22), (23000, 23)]}
POS = "wav2vec2.encoder.pos_conv_embed.conv"
HEADS = ("rich", "peaked")
RICH_SEED = {"tiny": 129, "large": 296}
PEAKED = {"tiny": (15, 0.5, 2.0, 0), "large": (30, 0.9, 0.5, 1)}  # (seed, rho, blank bias, the delimiter's rank) per geometry
PEAKED_SCALE = 4.0


def hf_config(cfg) -> dict:
    """The geometry as a transformers config.json."""
    return {"model_type": "wav2vec2", "architectures": ["Wav2Vec2ForCTC"], "feat_extract_norm": "layer",
            "do_stable_layer_norm": True, "conv_bias": True, "feat_extract_activation": "gelu", "hidden_act": "gelu",
            "conv_dim": [c for c, _, _ in cfg["conv"]], "conv_kernel": [k for _, k, _ in cfg["conv"]],
            "conv_stride": [s for _, _, s in cfg["conv"]], "hidden_size": cfg["embed"],
            "num_hidden_layers": cfg["layers"], "num_attention_heads": cfg["heads"], "intermediate_size": cfg["ffn"],
            "num_conv_pos_embeddings": cfg["conv_pos"], "num_conv_pos_embedding_groups": cfg["conv_pos_groups"],
            "vocab_size": cfg["vocab"], "pad_token_id": 0, "layer_norm_eps": 1e-5, "num_feat_extract_layers": len(cfg["conv"])}


def state_dict_shapes(cfg) -> List[Tuple[str, Tuple[int, ...]]]:
    out: List[Tuple[str, Tuple[int, ...]]] = []
    cin = 1
    for i, (c, k, _) in enumerate(cfg["conv"]):
        p = f"wav2vec2.feature_extractor.conv_layers.{i}"
        out += [(p + ".conv.weight", (c, cin, k)), (p + ".conv.bias", (c,)), (p + ".layer_norm.weight", (c,)),
                (p + ".layer_norm.bias", (c,))]
        cin = c
    E, Fd = cfg["embed"], cfg["ffn"]
    out += [("wav2vec2.feature_projection.layer_norm.weight", (cin,)), ("wav2vec2.feature_projection.layer_norm.bias", (cin,)),
            ("wav2vec2.feature_projection.projection.weight", (E, cin)), ("wav2vec2.feature_projection.projection.bias", (E,)),
            (POS + ".bias", (E,)), (POS + ".weight_g", (1, 1, cfg["conv_pos"])),
            (POS + ".weight_v", (E, E // cfg["conv_pos_groups"], cfg["conv_pos"]))]
    for l in range(cfg["layers"]):
        p = f"wav2vec2.encoder.layers.{l}"
        for q in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += [(f"{p}.attention.{q}.weight", (E, E)), (f"{p}.attention.{q}.bias", (E,))]
        out += [(p + ".layer_norm.weight", (E,)), (p + ".layer_norm.bias", (E,)),
                (p + ".feed_forward.intermediate_dense.weight", (Fd, E)), (p + ".feed_forward.intermediate_dense.bias", (Fd,)),
                (p + ".feed_forward.output_dense.weight", (E, Fd)), (p + ".feed_forward.output_dense.bias", (E,)),
                (p + ".final_layer_norm.weight", (E,)), (p + ".final_layer_norm.bias", (E,))]
    out += [("wav2vec2.encoder.layer_norm.weight", (E,)), ("wav2vec2.encoder.layer_norm.bias", (E,)),
            ("lm_head.weight", (cfg["vocab"], E)), ("lm_head.bias", (cfg["vocab"],))]
    return out


def synth_state(cfg) -> Dict[str, torch.Tensor]:
    sd: Dict[str, torch.Tensor] = {}
    for i, (name, shape) in enumerate(state_dict_shapes(cfg)):
        g = torch.Generator().manual_seed(SEED0 + i)
        if name.endswith("weight_g"):
            # ||v[:, :, k]|| ~ sqrt(E * E/G) and fan_in = E/G * taps: g = U(0.5, 1.5) sqrt(E / taps) gives an effective weight of
            # variance ~1 / fan_in
            sd[name] = (0.5 + torch.rand(shape, generator=g)) * (cfg["embed"] / cfg["conv_pos"]) ** 0.5
        elif name.endswith("layer_norm.weight"):
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            sd[name] = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 3:
            gain = 1.0 if name.endswith("weight_v") else (2.0 / (shape[1] * shape[2])) ** 0.5
            sd[name] = gain * torch.randn(shape, generator=g)
        else:
            w = torch.randn(shape, generator=g) / shape[1] ** 0.5
            if name.endswith("out_proj.weight") or name.endswith("output_dense.weight"):
                w = BRANCH_SCALE * w
            if name == "lm_head.weight":
                w = LM_SCALE * w
            sd[name] = w
    sd["lm_head.bias"][0] += LM_BLANK_BIAS
    return sd


def rich_head(name: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lm_head.weight, lm_head.bias) of the geometry's rich head: 32 like-scaled rows from ``RICH_SEED[name]``, chosen so
    that the word delimiter occurs inside a transcript, at an utterance's edge and twice in a row around a blank."""
    E = CONFIGS[name]["embed"]
    g = torch.Generator().manual_seed(RICH_SEED[name])
    W = LM_SCALE * torch.randn(32, E, generator=g) / E ** 0.5
    b = 0.1 * torch.randn(32, generator=g)
    b[0] += LM_BLANK_BIAS
    return W, b


def peaked_head(name: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lm_head.weight, lm_head.bias) of the geometry's peaked head (module docstring)."""
    seed, rho, bb, delim_rank = PEAKED[name]
    E = CONFIGS[name]["embed"]
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(32, E, generator=g) / E ** 0.5
    b = 0.1 * torch.randn(32, generator=g)
    perm = torch.randperm(27, generator=g)
    sc = torch.zeros(32)
    sc[5:] = torch.tensor([rho ** r for r in range(28) if r != delim_rank])[perm]
    sc[4] = rho ** delim_rank
    b[0] += bb
    b[1:4] -= 6.0
    return PEAKED_SCALE * W * sc[:, None], b


def with_head(sd: Dict[str, torch.Tensor], name: str, head: str) -> Dict[str, torch.Tensor]:
    """The geometry's state with the given head."""
    out = dict(sd)
    out["lm_head.weight"], out["lm_head.bias"] = rich_head(name) if head == "rich" else peaked_head(name)
    return out


def synth_audio(n: int, seed: int, rate: int = 16000) -> torch.Tensor:
    """[n] speech-like test signal: five slowly amplitude-modulated tones below 3.5 kHz on a noise floor, peak ~0.5, with a
    small DC offset (the normalisation has a mean to remove)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / rate
    f = 100.0 + 3400.0 * torch.rand(5, generator=g, dtype=torch.float64)
    ph = 6.283185307179586 * torch.rand(5, generator=g, dtype=torch.float64)
    mod = 2.0 + 6.0 * torch.rand(5, generator=g, dtype=torch.float64)
    x = (torch.sin(6.283185307179586 * f[:, None] * t[None] + ph[:, None]) *
         (0.5 + 0.5 * torch.sin(6.283185307179586 * mod[:, None] * t[None]))).sum(0) / 5.0
    x = x + 0.02 * torch.randn(n, generator=g, dtype=torch.float64) + 0.01
    return (0.5 * x).float()


def frame_count(cfg, n: int) -> int:
    for _, k, s in cfg["conv"]:
        n = 0 if n < k else (n - k) // s + 1
    return n


def fold_pos(sd) -> torch.Tensor:
    g, v = sd[POS + ".weight_g"].double(), sd[POS + ".weight_v"].double()
    return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()


def restated_forward(sd: Dict[str, torch.Tensor], cfg, wave: torch.Tensor, upto: str = "logits") -> torch.Tensor:
    """float64 forward of ONE utterance: wave [n] -> logits [T, vocab]."""
    w = {k: v.double() for k, v in sd.items()}
    x = wave.double()
    x = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)
    x = x[None, None]
    for i, (c, k, s) in enumerate(cfg["conv"]):
        p = f"wav2vec2.feature_extractor.conv_layers.{i}"
        x = F.conv1d(x, w[p + ".conv.weight"], w[p + ".conv.bias"], stride=s)
        x = F.layer_norm(x.transpose(1, 2), (c,), w[p + ".layer_norm.weight"], w[p + ".layer_norm.bias"], 1e-5).transpose(1, 2)
        x = F.gelu(x)
    x = x[0].t()  # [T, C]
    if upto == "features":
        return x
    C, E, H = x.shape[1], cfg["embed"], cfg["heads"]
    x = F.layer_norm(x, (C,), w["wav2vec2.feature_projection.layer_norm.weight"], w["wav2vec2.feature_projection.layer_norm.bias"], 1e-5)
    x = F.linear(x, w["wav2vec2.feature_projection.projection.weight"], w["wav2vec2.feature_projection.projection.bias"])
    kp = cfg["conv_pos"]
    pos = F.conv1d(x.t()[None], fold_pos(sd), w[POS + ".bias"], padding=kp // 2, groups=cfg["conv_pos_groups"])
    if kp % 2 == 0:
        pos = pos[:, :, :-1]
    x = x + F.gelu(pos[0].t())
    T, dh = x.shape[0], E // H
    for l in range(cfg["layers"]):
        p = f"wav2vec2.encoder.layers.{l}"
        h = F.layer_norm(x, (E,), w[p + ".layer_norm.weight"], w[p + ".layer_norm.bias"], 1e-5)
        q = F.linear(h, w[p + ".attention.q_proj.weight"], w[p + ".attention.q_proj.bias"]).view(T, H, dh).transpose(0, 1)
        k = F.linear(h, w[p + ".attention.k_proj.weight"], w[p + ".attention.k_proj.bias"]).view(T, H, dh).transpose(0, 1)
        v = F.linear(h, w[p + ".attention.v_proj.weight"], w[p + ".attention.v_proj.bias"]).view(T, H, dh).transpose(0, 1)
        a = torch.softmax(q @ k.transpose(1, 2) * dh ** -0.5, dim=-1) @ v
        x = x + F.linear(a.transpose(0, 1).reshape(T, E), w[p + ".attention.out_proj.weight"], w[p + ".attention.out_proj.bias"])
        h = F.layer_norm(x, (E,), w[p + ".final_layer_norm.weight"], w[p + ".final_layer_norm.bias"], 1e-5)
        h = F.gelu(F.linear(h, w[p + ".feed_forward.intermediate_dense.weight"], w[p + ".feed_forward.intermediate_dense.bias"]))
        x = x + F.linear(h, w[p + ".feed_forward.output_dense.weight"], w[p + ".feed_forward.output_dense.bias"])
    x = F.layer_norm(x, (E,), w["wav2vec2.encoder.layer_norm.weight"], w["wav2vec2.encoder.layer_norm.bias"], 1e-5)
    return F.linear(x, w["lm_head.weight"], w["lm_head.bias"])


def collapse(frame_ids, blank: int = 0) -> List[int]:
    """Greedy CTC: merge repeats, drop the blank."""
    out, prev = [], None
    for i in frame_ids:
        i = int(i)
        if i != prev and i != blank:
            out.append(i)
        prev = i
    return out


def ids_to_text(ids, vocab=VOCAB) -> str:
    inv = {i: t for t, i in vocab.items()}
    return "".join(" " if inv[int(i)] == "|" else inv[int(i)] for i in ids).strip()


def fingerprints(sd):
    """(checksums, first four values) per tensor: what the golden stores so that a test can prove it regenerated the same
    weights.  The checksum is the int64 sum of the fp32 bit patterns: exact and independent of the order of summation (a
    float sum's last bits change with the machine's vector width and thread count)."""
    import numpy as np
    sums = np.array([int(v.contiguous().view(torch.int32).to(torch.int64).sum()) for v in sd.values()], np.int64)
    first = np.stack([np.pad(v.flatten()[:4].double().numpy(), (0, 4 - min(4, v.numel())), constant_values=np.nan)
                      for v in sd.values()])
    return sums, first
