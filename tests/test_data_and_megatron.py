"""Data helpers (C++ runtime vs Python twins, mmap indexed dataset) and the Megatron recipe
surface: NB3's hyperparameters parse with the verbatim flag names, derived sizes, and a tiny
pretrain_gpt run that checkpoints and resumes in the Megatron layout."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from smdt_amd import _runtime
from smdt_amd.data import gpt_dataset as G
from smdt_amd.data import indexed_dataset as I

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cpp_sample_idx_matches_python_twin(seed):
    rng = np.random.RandomState(seed)
    sizes = rng.randint(1, 300, size=400).astype(np.int32)
    docs = np.arange(len(sizes), dtype=np.int32)
    epochs, seq = 3, 128
    doc_idx = G.build_doc_idx(docs, epochs, rng, False).astype(np.int32)
    tpe = int(sizes.sum())
    a = _runtime.build_sample_idx(sizes, doc_idx, seq, epochs, tpe)
    b = G.build_sample_idx_py(sizes, doc_idx, seq, epochs, tpe)
    np.testing.assert_array_equal(np.asarray(a), b)


def test_cpp_blending_indices_track_weights():
    w = np.array([0.5, 0.3, 0.2])
    d, s = _runtime.build_blending_indices(w, 1000)
    d, s = np.asarray(d), np.asarray(s)
    counts = np.bincount(d, minlength=3)
    np.testing.assert_allclose(counts / 1000, w, atol=2e-3)
    for k in range(3):  # per-dataset sample indices are 0..count-1 in order
        np.testing.assert_array_equal(s[d == k], np.arange(counts[k]))


def test_mmap_indexed_dataset_roundtrip(tmp_path):
    prefix = str(tmp_path / "corpus_text_document")
    I.write_synthetic_corpus(prefix, num_docs=50, vocab_size=1000, mean_len=40, seed=3)
    ds = I.make_dataset(prefix, "mmap")
    assert len(ds) == 50
    assert ds.sizes.sum() == sum(len(ds[i]) for i in range(50))
    assert all(int(ds[i][-1]) == 999 for i in range(50))  # every document ends with EOD


def test_gpt_dataset_samples_and_index_cache(tmp_path):
    prefix = str(tmp_path / "c_text_document")
    I.write_synthetic_corpus(prefix, num_docs=200, vocab_size=500, mean_len=60, seed=4)
    tr, va, te = G.build_train_valid_test_datasets([prefix], "mmap", "949,50,1", [64, 8, 8], 32, 1234, True)
    x = tr[0]["text"]
    assert x.shape == (33,) and len(tr) >= 64
    cache = [f for f in os.listdir(tmp_path / "index-cache") if f.endswith(".npy")] \
        if os.path.isdir(tmp_path / "index-cache") else [f for f in os.listdir(tmp_path) if f.endswith(".npy")]
    assert cache, "index mappings were not cached"
    tr2, _, _ = G.build_train_valid_test_datasets([prefix], "mmap", "949,50,1", [64, 8, 8], 32, 1234, True)
    np.testing.assert_array_equal(tr2[5]["text"], tr[5]["text"])


NB3 = {"num-layers": 12, "hidden-size": 768, "num-attention-heads": 12, "seq-length": 1024,
       "max-position-embeddings": 1024, "micro-batch-size": 12, "global-batch-size": 192, "lr": 0.0005,
       "train-iters": 4000, "lr-decay-iters": 150000, "lr-decay-style": "cosine", "lr-warmup-iters": 2000,
       "weight-decay": .1, "adam-beta2": .999, "fp16": "true", "log-interval": 10, "save-interval": 2000,
       "eval-interval": 200, "eval-iters": 10, "data-path": "/opt/ml/input/data/dataset/codeparrot_content_document",
       "vocab-file": "/opt/ml/input/data/dataset/gpt2-vocab.json",
       "merge-file": "/opt/ml/input/data/dataset/gpt2-merges.txt", "save": "/opt/ml/model/",
       "tensor-model-parallel-size": 4, "pipeline-model-parallel-size": 1}


def test_nb3_hyperparameters_parse_and_derive(monkeypatch):
    from smdt_amd.launch.hyperparameters import hyperparameters_to_cli
    from smdt_amd.train import arguments as A
    monkeypatch.setenv("WORLD_SIZE", "16")
    monkeypatch.setenv("RANK", "3")
    args = A.parse_args(argv=hyperparameters_to_cli(NB3))
    args = A.validate_args(args, {"tokenizer_type": "GPT2BPETokenizer"})
    assert args.data_parallel_size == 4 and args.num_micro_batches == 4
    assert args.fp16 is True and args.params_dtype == torch.float16
    assert args.tokenizer_type == "GPT2BPETokenizer"
    from smdt_amd.data.tokenizer import vocab_size_with_padding
    args.padded_vocab_size = vocab_size_with_padding(50257, args.make_vocab_size_divisible_by,
                                                     args.tensor_model_parallel_size)
    assert args.padded_vocab_size == 50688        # NB3:1212 "(50257 -> 50688)"
    cfg = A.core_transformer_config_from_args(args)
    assert (cfg.num_layers, cfg.hidden_size, cfg.num_attention_heads) == (12, 768, 12)


def test_every_reference_megatron_flag_parses(monkeypatch):
    """All 230 flag names of the reference's arguments.py (fixture tests/fixtures/
    megatron_reference_flags.json) parse in ONE command line; the task families this framework
    does not train (vision, biencoder / ICT, Retro, inference) are accepted, reported by
    ``ignored_flags_set`` and warned about by ``validate_args``."""
    import json
    import warnings
    from smdt_amd.train import arguments as A
    flags = json.load(open(os.path.join(REPO, "tests", "fixtures", "megatron_reference_flags.json")))["flags"]
    assert len(flags) == 230
    p = A.build_parser()
    by_flag = {o: a for a in p._actions for o in a.option_strings}
    skip = {"--batch-size", "--warmup", "--model-parallel-size", "--checkpoint-activations"}  # rejected later
    argv = []
    for f in flags:
        a = by_flag[f]                    # KeyError = a reference flag this parser does not know
        if f in skip:
            continue
        if a.nargs == 0:
            argv.append(f)
            continue
        if a.choices:
            v = str(list(a.choices)[0])
        elif a.type is int:
            v = "2"
        elif a.type is float:
            v = "0.5"
        elif a.type is A.str_bool:
            v = "true"
        else:
            v = "x"
        argv += [f, v]
    args = p.parse_args(argv)
    assert args.num_classes == 2 and args.dino_teacher_temp == 0.5 and args.retro_add_retriever is True
    assert args.data_sharding is False and args.retriever_report_topk_accuracies == [2]
    ign = A.ignored_flags_set(args)
    assert "--num-classes" in ign and "--retro-workdir" in ign and "--max-tokens-to-oom" in ign
    # defaults only: nothing to report; a non-default ignored flag warns in validate_args
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    base = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "32",
            "--max-position-embeddings", "32", "--micro-batch-size", "2"]
    assert A.ignored_flags_set(A.parse_args(argv=base)) == []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        A.validate_args(A.parse_args(argv=base + ["--img-h", "128", "--vision-pretraining"]),
                        {"tokenizer_type": "GPT2BPETokenizer"})
    msg = " ".join(str(x.message) for x in w)
    assert "--img-h" in msg and "--vision-pretraining" in msg
    # model-form flags without effect here warn too; --no-position-embedding drops the table
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        A.validate_args(A.parse_args(argv=base), {"tokenizer_type": "GPT2BPETokenizer"})
    assert not any("without effect" in str(x.message) for x in w)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = A.validate_args(A.parse_args(argv=base + ["--fp32-residual-connection", "--embedding-weights-in-fp32",
                                                      "--no-position-embedding", "--apply-layernorm-1p"]),
                            {"tokenizer_type": "GPT2BPETokenizer"})
    msg = " ".join(str(x.message) for x in w)
    assert "--fp32-residual-connection" in msg and "--embedding-weights-in-fp32" in msg
    assert "--no-position-embedding" not in msg and "--apply-layernorm-1p" not in msg
    assert a.position_embedding_type == "none"
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    a.padded_vocab_size = 64
    cfg = A.core_transformer_config_from_args(a)
    assert GPTModel(cfg).position_embeddings is None


@pytest.mark.slow
@pytest.mark.parametrize("async_save", [False, True])
def test_pretrain_gpt_checkpoint_and_resume(tmp_path, async_save):
    """Megatron layout save at --save-interval and resume; with --async-save the files are written
    by a background thread and the tracker only once the writers are done."""
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    common = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "64",
              "--max-position-embeddings", "64", "--micro-batch-size", "2", "--global-batch-size", "4",
              "--lr", "0.001", "--lr-decay-style", "cosine", "--lr-warmup-iters", "1", "--mock-data",
              "--log-interval", "1", "--eval-interval", "100", "--eval-iters", "1", "--save", str(tmp_path / "ck"),
              "--save-interval", "3", "--vocab-size", "512", "--tokenizer-type", "NullTokenizer"]
    if async_save:
        common.append("--async-save")
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29531")
    r = subprocess.run([sys.executable, script, "--train-iters", "3"] + common, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "iteration        3/       3" in r.stdout or "iteration 3/3" in r.stdout.replace("  ", " ")
    assert (tmp_path / "ck" / "latest_checkpointed_iteration.txt").read_text().strip() == "3"
    assert (tmp_path / "ck" / "iter_0000003" / "mp_rank_00" / "model_optim_rng.pt").exists()
    if async_save:
        assert "successfully saved checkpoint at iteration       3" in r.stdout and "(async)" in r.stdout
    r2 = subprocess.run([sys.executable, script, "--train-iters", "5", "--load", str(tmp_path / "ck")] + common,
                        env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-3000:]
    out = r2.stdout.replace("  ", " ")
    assert "iteration 4/" in " ".join(out.split()) and "iteration 1/" not in " ".join(out.split())


def test_load_without_optimizer_state_refreshes_masters(tmp_path):
    """weights loaded from a --no-save-optim checkpoint must reach the fp32 masters
    (the optimizer is built before the load), and the NumPy RNG state resumes too."""
    import argparse
    import numpy as np
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    from smdt_amd.train import checkpointing as ck
    ps.destroy_model_parallel()

    def build(seed):
        cfg = TransformerConfig(num_layers=1, hidden_size=32, num_attention_heads=2, max_position_embeddings=16,
                                padded_vocab_size=64, params_dtype=torch.float32, seed=seed)
        ddp = DistributedDataParallel(GPTModel(cfg))
        return ddp, MixedPrecisionAdam(ddp, lr=1e-3)
    ddp_a, opt_a = build(1)
    args = argparse.Namespace(save=str(tmp_path), load=str(tmp_path), no_save_optim=True)
    np.random.seed(123)
    ck.save_checkpoint(5, ddp_a, opt_a, None, args)
    want = np.random.rand(3)
    ddp_b, opt_b = build(2)
    assert not torch.equal(ddp_b.param_data, ddp_a.param_data)
    np.random.seed(999)
    assert ck.load_checkpoint(ddp_b, opt_b, None, args) == 5
    torch.testing.assert_close(ddp_b.param_data, ddp_a.param_data)
    for (s, e, _), mo in zip(opt_b.pieces, opt_b.master_off):
        torch.testing.assert_close(opt_b.master[mo:mo + e - s], ddp_a.param_data[s:e].float())
    np.testing.assert_array_equal(np.random.rand(3), want)


@pytest.mark.slow
def test_pretrain_gpt_fp16_applies_loss_scale(tmp_path):
    """--fp16: the schedules multiply the loss by the dynamic loss scale before backward (Megatron's
    optimizer.scale_loss) and the optimizer divides it back out — the reported grad norm is the
    unscaled one, an overflow step is skipped without corrupting the weights, and training
    continues with finite losses."""
    import re
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    args = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "64",
            "--max-position-embeddings", "64", "--micro-batch-size", "2", "--global-batch-size", "4",
            "--lr", "0.001", "--lr-warmup-iters", "1", "--mock-data", "--log-interval", "1", "--eval-interval",
            "100", "--eval-iters", "1", "--vocab-size", "512", "--tokenizer-type", "NullTokenizer",
            "--fp16", "true", "--train-iters", "4", "--initial-loss-scale", "4294967296", "--hysteresis", "1"]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    r = subprocess.run([sys.executable, script] + args, env=env, capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if "lm loss:" in ln and "iteration" in ln]
    assert len(lines) == 4
    losses = [float(re.search(r"lm loss: (\S+)", ln).group(1)) for ln in lines]
    scales = [float(re.search(r"loss scale: (\S+)", ln).group(1)) for ln in lines]
    norms = [re.search(r"grad norm: (\S+)", ln).group(1) for ln in lines]
    assert all(math.isfinite(x) for x in losses), lines
    assert scales[-1] < scales[0], scales            # overflowing steps halved the scale
    finite = [float(n) for n in norms if n not in ("nan", "inf")]
    assert all(n < 100 for n in finite), norms       # unscaled norms (scaled ones would be ~1e9)


@pytest.mark.slow
def test_pretrain_gpt_rampup_batch_size(tmp_path):
    """--rampup-batch-size 2 2 24 with --train-samples: the logged global batch size ramps 2 -> 4 -> 6
    -> 8 (micro-batches per step follow consumed samples) and training ends at the sample budget."""
    import re
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    args = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "64",
            "--max-position-embeddings", "64", "--micro-batch-size", "2", "--global-batch-size", "8",
            "--rampup-batch-size", "2", "2", "24", "--train-samples", "60", "--lr", "0.001",
            "--lr-warmup-samples", "24", "--lr-decay-style", "constant",
            "--mock-data", "--log-interval", "1", "--eval-interval", "1000", "--eval-iters", "1",
            "--vocab-size", "512", "--tokenizer-type", "NullTokenizer"]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29539")
    r = subprocess.run([sys.executable, script] + args, env=env, capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    gbs = [int(x) for x in re.findall(r"global batch size:\s+(\d+)", r.stdout)]
    cons = [int(x) for x in re.findall(r"consumed samples:\s+(\d+)", r.stdout)]
    assert gbs[0] == 2 and gbs[-1] == 8 and gbs == sorted(gbs) and {2, 4, 6, 8} <= set(gbs), gbs
    assert cons[-1] >= 60 and cons[-2] < 60, cons
    assert "batch size rampup starting from global batch size 2" in r.stdout
    # the LR warms up over 24 SAMPLES, stepped by each iteration's (ramping) global batch
    lrs = [float(x) for x in re.findall(r"learning rate:\s+([0-9.eE+-]+)", r.stdout)]
    assert abs(lrs[0] - 0.001 * 2 / 24) < 1e-7, lrs
    assert abs(lrs[1] - 0.001 * 4 / 24) < 1e-7, lrs   # batch 2 for the first 8 samples
    assert lrs[-1] == 0.001 and lrs == sorted(lrs), lrs


def test_tensorboard_event_file_format(tmp_path):
    """the dependency-free event writer emits CRC-32C-framed TFRecords holding
    tensorflow.Event protobufs (checked against the standard CRC-32C test vector and a parse-back)."""
    from smdt_amd.utils import tensorboard as tb
    assert tb.crc32c(b"123456789") == 0xE3069283
    w = tb.SummaryWriter(str(tmp_path), max_queue=2)
    for i in range(5):
        w.add_scalar("lm loss", 10.0 - i, i + 1)
    w.add_scalars("timers", {"fwd": 1.5, "bwd": 2.5}, 7)
    w.close()
    files = list(tmp_path.glob("events.out.tfevents.*"))
    assert len(files) == 1
    recs = list(tb.read_records(str(files[0])))
    assert b"brain.Event:2" in recs[0]
    sc = tb.read_scalars(str(files[0]))
    assert [(s, t) for s, t, _ in sc[:5]] == [(i + 1, "lm loss") for i in range(5)]
    assert [v for _, _, v in sc[:5]] == [10.0, 9.0, 8.0, 7.0, 6.0]
    assert ("timers/bwd", 2.5) in [(t, v) for _, t, v in sc]
    raw = files[0].read_bytes()
    bad = raw[:-1] + bytes([raw[-1] ^ 1])
    files[0].write_bytes(bad)
    with pytest.raises(ValueError):
        tb.read_scalars(str(files[0]))


@pytest.mark.slow
def test_pretrain_gpt_writes_tensorboard_and_runs_context_parallel(tmp_path):
    """--tensorboard-dir with the Megatron log flags writes learning-rate / lm loss / grad-norm /
    batch-size / timer scalars per iteration on the last rank; the run uses --context-parallel-size 2
    (world 2, gloo) so the CP batch slicing and dp x cp loss averaging run end to end."""
    from smdt_amd.utils import tensorboard as tb
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    args = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "64",
            "--max-position-embeddings", "64", "--micro-batch-size", "2", "--global-batch-size", "4",
            "--lr", "0.001", "--lr-warmup-iters", "1", "--mock-data", "--log-interval", "1",
            "--eval-interval", "2", "--eval-iters", "1", "--vocab-size", "512", "--tokenizer-type", "NullTokenizer",
            "--train-iters", "3", "--tensorboard-dir", str(tmp_path / "tb"), "--log-timers-to-tensorboard",
            "--log-batch-size-to-tensorboard", "--log-validation-ppl-to-tensorboard", "--context-parallel-size", "2",
            "--timing-log-level", "1",
            "--distributed-backend", "gloo"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29547", script] + args, env=env, capture_output=True,
                       text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "context-parallel size: 2" in r.stdout
    files = list((tmp_path / "tb").glob("events.out.tfevents.*"))
    assert len(files) == 1, files      # only the last rank writes
    sc = tb.read_scalars(str(files[0]))
    tags = {t for _, t, _ in sc}
    for want in ("learning-rate", "lm loss", "lm loss vs samples", "grad-norm", "batch-size",
                 "forward-backward-time", "lm loss validation", "lm loss validation ppl"):
        assert want in tags, (want, sorted(tags))
    steps = sorted(s for s, t, _ in sc if t == "lm loss")
    assert steps == [1, 2, 3]
    assert all(math.isfinite(v) for _, _, v in sc)


@pytest.mark.parametrize("offset", [0, 3])
def test_gpt_position_slice_matches_gathered_positions(offset):
    """Default positions (no position_ids) take the broadcast-slice path with a batch-sum
    backward into main_grad; explicit position_ids take the gather / scatter path. Same loss,
    same main_grad for every parameter."""
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=1, hidden_size=32, num_attention_heads=2, max_position_embeddings=16,
                            padded_vocab_size=64, params_dtype=torch.float32, seed=7, position_offset=offset,
                            hidden_dropout=0.0, attention_dropout=0.0)
    ddp = DistributedDataParallel(GPTModel(cfg))
    model = ddp.module if hasattr(ddp, "module") else ddp
    tok = torch.randint(0, 64, (3, 9))
    grads = []
    for pos in (None, torch.arange(8).unsqueeze(0).expand(3, 8)):
        ddp.zero_grad_buffer()
        loss = model(tok[:, :-1], position_ids=pos, labels=tok[:, 1:]).float().mean()
        loss.backward()
        ddp.finish_grad_sync()
        grads.append((loss.detach(), ddp.grad_data.clone()))
    torch.testing.assert_close(grads[0][0], grads[1][0])
    torch.testing.assert_close(grads[0][1], grads[1][1], rtol=1e-5, atol=1e-6)
    assert grads[0][1].abs().sum() > 0
    # Megatron's get_batch positions are marked as plain aranges (slice path); reset ones are not
    from smdt_amd.train.utils import get_ltor_masks_and_position_ids
    _, _, p_plain = get_ltor_masks_and_position_ids(tok[:, :-1], 0)
    _, _, p_reset = get_ltor_masks_and_position_ids(tok[:, :-1], 0, reset_position_ids=True)
    assert getattr(p_plain, "_smdt_arange_start", None) == 0
    assert getattr(p_reset, "_smdt_arange_start", None) is None


def test_async_save_snapshots_state_at_save_time(tmp_path):
    """--async-save: the files hold the state of the save call even when the weights change while
    the writer thread runs; the tracker appears only after finalize_async_save."""
    import argparse
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    from smdt_amd.train import checkpointing as ck
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=1, hidden_size=32, num_attention_heads=2, max_position_embeddings=16,
                            padded_vocab_size=64, params_dtype=torch.float32)
    ddp = DistributedDataParallel(GPTModel(cfg))
    opt = MixedPrecisionAdam(ddp, lr=1e-3)
    args = argparse.Namespace(save=str(tmp_path), async_save=True)
    want = {k: v.clone() for k, v in ddp.module.state_dict().items()}
    ck.save_checkpoint(7, ddp, opt, None, args)
    with torch.no_grad():
        for p in ddp.module.parameters():
            p.add_(1.0)                       # training goes on while the writer runs
    assert ck.finalize_async_save(blocking=True)
    assert (tmp_path / ck.TRACKER).read_text().strip() == "7"
    sd = torch.load(tmp_path / "iter_0000007" / "mp_rank_00" / "model_optim_rng.pt", weights_only=True)
    for k, v in want.items():
        assert torch.equal(sd["model"][k], v), k
    assert ck.finalize_async_save(blocking=False)   # nothing pending any more


@pytest.mark.slow
def test_pretrain_gpt_logs_params_norm_and_num_zeros(tmp_path):
    """--log-params-norm / --log-num-zeros-in-grad: every training-log line carries Megatron's
    ``num zeros: N |`` and ``params norm: X |`` fields (after the grad norm); the norm is finite,
    positive and moves with the updates, the zero count is a non-negative count."""
    import re
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    args = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "64",
            "--max-position-embeddings", "64", "--micro-batch-size", "2", "--global-batch-size", "4",
            "--lr", "0.01", "--lr-warmup-iters", "1", "--mock-data", "--log-interval", "1", "--eval-interval",
            "100", "--eval-iters", "1", "--vocab-size", "512", "--tokenizer-type", "NullTokenizer",
            "--train-iters", "3", "--log-params-norm", "--log-num-zeros-in-grad"]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    r = subprocess.run([sys.executable, script] + args, env=env, capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if "lm loss:" in ln and "iteration" in ln]
    assert len(lines) == 3, r.stdout[-2000:]
    pn = [float(re.search(r"params norm: (\S+) \|", ln).group(1)) for ln in lines]
    nz = [float(re.search(r"num zeros: (\S+) \|", ln).group(1)) for ln in lines]
    assert all(math.isfinite(x) and x > 0 for x in pn) and len(set(pn)) > 1, pn
    assert all(x >= 0 and x == int(x) for x in nz), nz
    assert all(ln.index("grad norm:") < ln.index("num zeros:") < ln.index("params norm:") for ln in lines)


def test_sgd_optimizer_matches_torch_sgd():
    """``--optimizer sgd``: MixedPrecisionSGD over the flat fp32 masters equals torch.optim.SGD
    (momentum, no dampening) on an identical copy of the model, step for step."""
    import copy
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionSGD
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=1, hidden_size=32, num_attention_heads=2, max_position_embeddings=16,
                            padded_vocab_size=64, params_dtype=torch.float32, hidden_dropout=0.0,
                            attention_dropout=0.0, seed=3)
    model = GPTModel(cfg)
    ref = copy.deepcopy(model)
    ddp = DistributedDataParallel(model)
    opt = MixedPrecisionSGD(ddp, lr=0.05, momentum=0.9)
    ropt = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9)
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        tok = torch.randint(0, 64, (2, 17), generator=g)
        ddp.zero_grad_buffer()
        ddp(tok[:, :-1], None, None, labels=tok[:, 1:]).float().mean().backward()
        ddp.finish_grad_sync()
        opt.step()
        ropt.zero_grad()
        ref(tok[:, :-1], None, None, labels=tok[:, 1:]).float().mean().backward()
        ropt.step()
    got = dict(model.named_parameters())
    for k, p in ref.named_parameters():
        torch.testing.assert_close(got[k], p, rtol=1e-5, atol=1e-6, msg=k)
    assert opt.exp_avg.abs().sum() > 0 and opt.exp_avg_sq.numel() == 0


def test_pretrain_gpt_optimizer_sgd_trains(tmp_path):
    """``--optimizer sgd --sgd-momentum 0.9`` reaches the SGD update (not Adam's): the run logs the
    optimizer it built and every logged loss is finite."""
    import re
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    args = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "64",
            "--max-position-embeddings", "64", "--micro-batch-size", "2", "--global-batch-size", "4",
            "--lr", "0.05", "--lr-warmup-iters", "0", "--mock-data", "--log-interval", "1", "--eval-interval",
            "100", "--eval-iters", "1", "--vocab-size", "512", "--tokenizer-type", "NullTokenizer",
            "--train-iters", "4", "--optimizer", "sgd", "--sgd-momentum", "0.9"]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29543")
    r = subprocess.run([sys.executable, script] + args, env=env, capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "optimizer: MixedPrecisionSGD" in r.stdout + r.stderr
    losses = [float(re.search(r"lm loss: (\S+) \|", ln).group(1)) for ln in r.stdout.splitlines()
              if "lm loss:" in ln and "iteration" in ln]
    assert len(losses) == 4 and all(math.isfinite(x) for x in losses), losses


def test_pretrain_gpt_use_checkpoint_args(tmp_path):
    """``--use-checkpoint-args``: a resumed run given a different model shape on its command line
    takes the checkpoint's (num layers, hidden size, heads) and loads it strictly; without the flag
    the same command line cannot load that checkpoint."""
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    common = ["--seq-length", "32", "--max-position-embeddings", "32", "--micro-batch-size", "2",
              "--global-batch-size", "2", "--lr", "0.01", "--mock-data", "--log-interval", "1",
              "--eval-interval", "100", "--eval-iters", "1", "--vocab-size", "256", "--tokenizer-type",
              "NullTokenizer", "--save-interval", "2"]
    first = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--train-iters", "2",
             "--save", str(tmp_path / "ck")]
    other = ["--num-layers", "3", "--hidden-size", "32", "--num-attention-heads", "2", "--train-iters", "3",
             "--load", str(tmp_path / "ck")]

    def run(extra, port):
        env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        return subprocess.run([sys.executable, script] + common + extra, env=env, capture_output=True,
                              text=True, timeout=600, cwd=str(tmp_path))
    r = run(first, 29545)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    r = run(other + ["--use-checkpoint-args"], 29546)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "successfully loaded checkpoint" in r.stdout and "iteration        3/" in r.stdout, r.stdout[-2000:]
    r = run(other, 29547)
    assert r.returncode != 0


def test_xavier_init_and_no_initialization():
    """``--init-method-xavier-uniform`` draws every 2-D weight from U(-a, a), a = sqrt(6 / (fan_in +
    fan_out)) of the full weight; ``--no-initialization`` builds the model without drawing (the
    checkpoint load fills it); the default stays N(0, init_method_std)."""
    import math as _m
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    from smdt_amd.train import arguments as A
    ps.destroy_model_parallel()
    base = dict(num_layers=1, hidden_size=64, num_attention_heads=4, max_position_embeddings=32,
                padded_vocab_size=128, params_dtype=torch.float32, ffn_hidden_size=256)
    xa = GPTModel(TransformerConfig(init_method="xavier_uniform", **base))
    nm = GPTModel(TransformerConfig(**base))
    for (k, p), (_, q) in zip(xa.named_parameters(), nm.named_parameters()):
        if p.dim() != 2:
            continue
        a = _m.sqrt(6.0 / (p.shape[0] + p.shape[1]))
        assert p.abs().max() <= a and p.abs().max() > 0.9 * a, k      # bounded by, and fills, [-a, a]
        assert abs(p.std().item() - a / _m.sqrt(3)) < 0.1 * a, k
        assert 0 < q.std().item() < 0.022, k                         # N(0, std) (scaled on outputs)
    un = GPTModel(TransformerConfig(perform_initialization=False, **base))
    assert [p.shape for p in un.parameters()] == [p.shape for p in nm.parameters()]
    argv = ["--num-layers", "1", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "32",
            "--max-position-embeddings", "32", "--micro-batch-size", "2", "--init-method-xavier-uniform",
            "--no-initialization"]
    old = {k: os.environ.get(k) for k in ("WORLD_SIZE", "RANK")}
    os.environ.update(WORLD_SIZE="1", RANK="0")
    try:
        a = A.validate_args(A.parse_args(argv=argv), {"tokenizer_type": "GPT2BPETokenizer"})
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    a.padded_vocab_size = 128
    cfg = A.core_transformer_config_from_args(a)
    assert cfg.init_method == "xavier_uniform" and cfg.perform_initialization is False


def test_layernorm_1p_and_post_layernorm_residual():
    """``--apply-layernorm-1p``: gamma is stored centred on zero and the norm scales by 1 + gamma
    (same output as the standard norm at init, gradient lands on the stored tensor).
    ``--apply-residual-connection-post-layernorm``: each sub-block's residual is the norm's OUTPUT,
    checked against the layer's own modules composed by hand (eval mode, no dropout)."""
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import ParallelTransformerLayer, TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    base = dict(num_layers=1, hidden_size=64, num_attention_heads=4, max_position_embeddings=32,
                padded_vocab_size=128, params_dtype=torch.float32, hidden_dropout=0.0, attention_dropout=0.0)
    tok = torch.randint(0, 128, (2, 17), generator=torch.Generator().manual_seed(0))
    std = GPTModel(TransformerConfig(seed=5, **base)).eval()
    onep = GPTModel(TransformerConfig(seed=5, layernorm_zero_centered_gamma=True, **base)).eval()
    w = onep.decoder.layers[0].input_norm.weight
    assert torch.equal(w, torch.zeros_like(w))
    l0 = std(tok[:, :-1], None, None, labels=tok[:, 1:]).float().mean()
    l1 = onep(tok[:, :-1], None, None, labels=tok[:, 1:]).float().mean()
    torch.testing.assert_close(l1, l0)
    l1.backward()
    assert w.grad is not None and w.grad.abs().sum() > 0
    with torch.no_grad():
        w.add_(0.5)                                   # scale 1.5: the output changes
    assert not torch.allclose(onep(tok[:, :-1], None, None, labels=tok[:, 1:]).float().mean(), l0)

    cfg = TransformerConfig(seed=7, apply_residual_connection_post_layernorm=True, **base)
    layer = ParallelTransformerLayer(cfg, 1).eval()
    x = torch.randn(16, 2, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        m, mb, res = layer(x, None, None)
        ln1 = layer.input_norm(x)
        a, ab = layer.attention(ln1, False)
        ln2 = layer.post_attention_norm(ln1 + a + (ab if ab is not None else 0))
        m2, mb2 = layer.mlp(ln2)
    torch.testing.assert_close(res, ln2)
    torch.testing.assert_close(m, m2)
    model = GPTModel(TransformerConfig(seed=7, apply_residual_connection_post_layernorm=True, **base))
    loss = model(tok[:, :-1], None, None, labels=tok[:, 1:]).float().mean()
    loss.backward()
    assert torch.isfinite(loss) and all(p.grad is not None for p in model.parameters() if p.requires_grad)


def test_switch_mlp_routes_each_token_to_one_expert():
    """``--num-experts``: every token's MLP output is (its top-1 expert's output + bias) x the
    router probability, checked token by token; gradients reach the router and every expert that
    received tokens; a GPT with experts trains a step through DDP + the optimizer."""
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import SwitchMLP, TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    from smdt_amd.train import arguments as A
    ps.destroy_model_parallel()
    base = dict(num_layers=2, hidden_size=32, num_attention_heads=2, max_position_embeddings=32,
                padded_vocab_size=64, params_dtype=torch.float32, hidden_dropout=0.0, attention_dropout=0.0,
                num_experts=4, seed=2)
    cfg = TransformerConfig(**base)
    mlp = SwitchMLP(cfg, 1)
    with torch.no_grad():
        mlp.router.mul_(50)                              # spread the routing over the experts
    x = torch.randn(8, 3, 32, generator=torch.Generator().manual_seed(0), requires_grad=True)
    out, bias = mlp(x)
    assert bias is None and out.shape == x.shape
    p, e = mlp.route(x.detach().reshape(-1, 32))
    assert len(set(e.tolist())) > 1
    for t in range(24):
        y, yb = mlp.experts[int(e[t])](x.detach().reshape(-1, 32)[t].view(1, 1, 32))
        want = (y + yb).view(32) * p[t]
        torch.testing.assert_close(out.reshape(-1, 32)[t], want, rtol=1e-5, atol=1e-6)
    out.square().sum().backward()
    assert mlp.router.grad is not None and mlp.router.grad.abs().sum() > 0
    for i, ex in enumerate(mlp.experts):
        if (e == i).any():
            assert ex.fc1.weight.grad is not None or getattr(ex.fc1.weight, "main_grad", None) is not None
    model = GPTModel(TransformerConfig(**base))
    assert sum(1 for n, _ in model.named_parameters() if ".experts." in n) > 0
    ddp = DistributedDataParallel(model)
    opt = MixedPrecisionAdam(ddp, lr=1e-2)
    tok = torch.randint(0, 64, (2, 17), generator=torch.Generator().manual_seed(1))
    before = ddp.param_data.clone()
    ddp.zero_grad_buffer()
    ddp(tok[:, :-1], None, None, labels=tok[:, 1:]).float().mean().backward()
    ddp.finish_grad_sync()
    opt.step()
    assert not torch.equal(before, ddp.param_data)
    argv = ["--num-layers", "1", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "32",
            "--max-position-embeddings", "32", "--micro-batch-size", "2", "--num-experts", "8"]
    old = {k: os.environ.get(k) for k in ("WORLD_SIZE", "RANK")}
    os.environ.update(WORLD_SIZE="1", RANK="0")
    try:
        a = A.validate_args(A.parse_args(argv=argv), {"tokenizer_type": "GPT2BPETokenizer"})
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    a.padded_vocab_size = 128
    assert A.core_transformer_config_from_args(a).num_experts == 8


def test_empty_unused_memory_level_and_grad_accum_fusion_flags(monkeypatch):
    """``--empty-unused-memory-level`` 1 empties the allocator cache after forward-backward (and
    eval iterations), 2 also after the optimizer step; ``--no-gradient-accumulation-fusion`` turns
    the MFMA wgrad-into-main_grad path off; ``--use-cpu-initialization`` reaches the config."""
    import argparse
    from smdt_amd.parallel import dense
    from smdt_amd.train import arguments as A
    from smdt_amd.train import training as T
    calls = []
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_available", lambda: True)
        m.setattr(torch.cuda, "empty_cache", lambda: calls.append(1))
        for level, want in ((0, 0), (1, 1), (2, 2)):
            calls.clear()
            a = argparse.Namespace(empty_unused_memory_level=level)
            T.empty_unused_memory(a, 1)
            T.empty_unused_memory(a, 2)
            assert len(calls) == want, (level, calls)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    argv = ["--num-layers", "1", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "32",
            "--max-position-embeddings", "32", "--micro-batch-size", "2", "--no-gradient-accumulation-fusion",
            "--use-cpu-initialization", "--empty-unused-memory-level", "2"]
    a = A.validate_args(A.parse_args(argv=argv), {"tokenizer_type": "GPT2BPETokenizer"})
    assert a.gradient_accumulation_fusion is False and a.empty_unused_memory_level == 2
    a.padded_vocab_size = 128
    assert A.core_transformer_config_from_args(a).use_cpu_initialization is True
    monkeypatch.setattr(dense, "_FUSED_WGRAD", True)
    class _Stop(Exception):
        pass

    def provider(**kw):
        raise _Stop                 # only the flag handling before the model build is under test
    with pytest.raises(_Stop):
        T.setup_model_and_optimizer(provider, a)
    assert dense._FUSED_WGRAD is False
