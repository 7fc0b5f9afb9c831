"""``python -m s2st_amd.average_checkpoints`` (stage 6 of the recipes; scripts/average_checkpoints.py +
examples/s2s_trans/convert_pt_to512.py of the reference) on three checkpoints derived from tests/golden/ckpt_nano.pt
(tests/ckpt_avg_fixture.py).

The reference's own script WAS run on those three files (tools/gen_golden_ckpt_avg.py, with oracle/ref_shims on the path);
its output is tests/golden/ckpt_avg.npz and ``test_average_equals_the_reference_scripts_output`` compares against it
exactly."""
import argparse
import importlib
import os

import numpy as np
import pytest
import torch

from ckpt_avg_fixture import TRACKED, make_inputs

PKG = "speech-to-speech-translation_amd"
U = 2.0 ** -24  # unit roundoff of fp32, round to nearest


def _avg():
    return importlib.import_module(PKG + ".average_checkpoints")


def _load(p):
    return torch.load(p, map_location="cpu", weights_only=False)


def test_average_against_float64_restatement(golden_dir, tmp_path):
    """fp32 accumulation s1 = fl(a + b), s2 = fl(s1 + c), q = fl(s2 / 3) against (a + b + c) / 3 in float64: the two sums
    err by at most u |a + b| and u |s2| (relative rounding, |s2| <= |a + b + c| (1 + u) + u |a + b|), both divided by 3, and
    the division by at most u |q|: the bound below, per element, from the partial sums' magnitudes (1.001: the second-order
    terms; 1e-44: a result in the subnormal range rounds absolutely)."""
    A = _avg()
    paths = make_inputs(golden_dir, str(tmp_path / "in"))
    out = str(tmp_path / "avg.pt")
    A.main(["--inputs"] + paths + ["--output", out])
    got, ins = _load(out), [_load(p) for p in paths]
    assert ins[1]["model"][next(iter(ins[1]["model"]))].dtype == torch.float16  # (the half file really is half)
    assert list(got["model"].keys()) == list(ins[0]["model"].keys())
    n_float = n_int = 0
    for k, v in got["model"].items():
        a, b, c = (s["model"][k] for s in ins)
        if not a.is_floating_point():
            assert v.dtype == a.dtype and v.tolist() == (np.asarray(sum(TRACKED)) // 3).tolist() == 8, k  # 26 // 3, not 8.67
            n_int += 1
            continue
        assert v.dtype == torch.float32, k
        a, b, c = (x.double().numpy() for x in (a, b, c))
        s1, s2 = np.abs(a + b), np.abs(a + b + c)
        bound = 1.001 * U * ((s1 + s2) / 3 + s2 / 3) + 1e-44
        want = (a + b + c) / 3
        ok = np.isfinite(want)  # (the sinusoidal position tables' one-element placeholder buffer is uninitialised memory)
        err = np.abs(v.double().numpy()[ok] - want[ok])
        assert (err <= bound[ok]).all(), (k, float(err.max()))
        assert np.array_equal(np.isnan(v.numpy()[~ok]), np.isnan(want[~ok])), k
        n_float += 1
    assert n_float > 100 and n_int >= 2
    # everything but the model is the first listed file's
    assert got["extra_state"]["which_file"] == 0
    assert set(got) == set(ins[0]) and got["optimizer_history"] == ins[0]["optimizer_history"]
    A.main(["--inputs"] + paths[::-1] + ["--output", out])
    assert _load(out)["extra_state"]["which_file"] == 2


def test_average_equals_the_reference_scripts_output(golden_dir, tmp_path):
    A = _avg()
    z = np.load(os.path.join(golden_dir, "ckpt_avg.npz"))
    d = str(tmp_path / "in")
    make_inputs(golden_dir, d)
    out = str(tmp_path / "avg.pt")
    A.main(["--inputs", d, "--num-epoch-checkpoints", "3", "--output", out])
    got = _load(out)
    assert z["order"].tolist() == ["checkpoint5.pt", "checkpoint4.pt", "checkpoint3.pt"]
    assert got["extra_state"]["which_file"] == int(z["which_file"]) == 2
    keys = [k[6:] for k in z.files if k.startswith("model.")]
    assert keys == list(got["model"].keys())
    for k in keys:
        v = got["model"][k].numpy()
        assert v.dtype == z["model." + k].dtype and np.array_equal(v, z["model." + k]), k


def _touch(d, names):
    os.makedirs(d, exist_ok=True)
    for n in names:
        open(os.path.join(d, n), "w").close()


def test_file_selection_rules(tmp_path):
    A = _avg()
    d = str(tmp_path / "stubs")
    _touch(d, ["checkpoint1.pt", "checkpoint2.pt", "checkpoint10.pt", "checkpoint9.pt", "checkpoint_last.pt", "checkpoint_best.pt",
               "checkpoint_3_500.pt", "checkpoint_3_1000.pt", "checkpoint_4_1500.pt", "checkpoint_12_20.pt", "xcheckpoint3.pt",
               "checkpoint3.pt.tmp"])
    base = lambda ps: [os.path.basename(p) for p in ps]  # noqa: E731
    assert base(A.last_n_checkpoints([d], 3, False)) == ["checkpoint10.pt", "checkpoint9.pt", "checkpoint2.pt"]  # by number
    assert base(A.last_n_checkpoints([d], 2, False, upper_bound=9)) == ["checkpoint9.pt", "checkpoint2.pt"]
    assert base(A.last_n_checkpoints([d], 4, False)) == ["checkpoint10.pt", "checkpoint9.pt", "checkpoint2.pt", "checkpoint1.pt"]
    assert base(A.last_n_checkpoints([d], 2, True)) == ["checkpoint_4_1500.pt", "checkpoint_3_1000.pt"]  # by update number
    assert base(A.last_n_checkpoints([d], 2, True, upper_bound=1000)) == ["checkpoint_3_1000.pt", "checkpoint_3_500.pt"]
    assert base(A.last_n_checkpoints([d], 4, True)) == ["checkpoint_4_1500.pt", "checkpoint_3_1000.pt", "checkpoint_3_500.pt",
                                                        "checkpoint_12_20.pt"]
    with pytest.raises(Exception, match="need at least 5"):
        A.last_n_checkpoints([d], 5, False)
    with pytest.raises(Exception, match="need at least 4"):  # (three of the update files lie at or below the bound)
        A.last_n_checkpoints([d], 4, True, upper_bound=1000)
    with pytest.raises(SystemExit):  # an upper bound without a count
        A.main(["--inputs", d, "--output", str(tmp_path / "o.pt"), "--checkpoint-upper-bound", "3"])
    with pytest.raises(SystemExit):  # the two counts exclude each other
        A.main(["--inputs", d, "--output", str(tmp_path / "o.pt"), "--num-epoch-checkpoints", "2", "--num-update-checkpoints", "2"])


def test_mismatching_keys_raise(golden_dir, tmp_path):
    A = _avg()
    paths = make_inputs(golden_dir, str(tmp_path / "in"))
    st = _load(paths[2])
    k0 = next(iter(st["model"]))
    st["model"]["renamed." + k0] = st["model"].pop(k0)
    torch.save(st, paths[2])
    with pytest.raises(KeyError):
        A.main(["--inputs"] + paths + ["--output", str(tmp_path / "o.pt")])
    st = _load(paths[1])  # the same keys in another order are a mismatch too
    items = list(st["model"].items())
    st["model"] = type(st["model"])(items[1:] + items[:1])
    torch.save(st, paths[1])
    with pytest.raises(KeyError):
        A.main(["--inputs"] + paths[:2] + ["--output", str(tmp_path / "o.pt")])


def test_decoder_embed_dim_patch_and_loading(backend, golden_dir, tmp_path):
    """--decoder-embed-dim sets cfg["model"].decoder_embed_dim and nothing else; the unpatched output loads through
    checkpoint_utils.load_checkpoint_to_cpu and model.load_state_dict(strict=True) into the model its cfg describes."""
    import s2st_oracle as O
    from ckpt_fixture import CKPT_CFG
    A = _avg()
    C = importlib.import_module(PKG + ".checkpoint_utils")
    paths = make_inputs(golden_dir, str(tmp_path / "in"))
    out, out512 = str(tmp_path / "avg.pt"), str(tmp_path / "avg512.pt")
    A.main(["--inputs"] + paths + ["--output", out])
    A.main(["--inputs"] + paths + ["--output", out512, "--decoder-embed-dim", "512"])
    st, st512 = C.load_checkpoint_to_cpu(out), C.load_checkpoint_to_cpu(out512)
    assert isinstance(st512["cfg"]["model"], argparse.Namespace)
    assert st["cfg"]["model"].decoder_embed_dim == 8 and st512["cfg"]["model"].decoder_embed_dim == 512
    a, b = vars(st["cfg"]["model"]), vars(st512["cfg"]["model"])
    assert {k for k in a if a[k] != b[k]} == {"decoder_embed_dim"}
    assert all(torch.equal(st["model"][k], st512["model"][k]) for k in st["model"])
    tasks = importlib.import_module(PKG + ".tasks")
    args = O.make_args(**CKPT_CFG)
    args.precise_gemm = True
    task = tasks.S2ST_TranslationTask.setup_task(args, device=backend.device)
    model = task.build_model(args)
    model.load_state_dict(st["model"], strict=True)
    k = "decoder.postnet.convolutions.0.1.num_batches_tracked"
    assert int(model.state_dict()[k]) == 8
