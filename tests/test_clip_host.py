"""No-GPU checks of the per-clip attack: the new C-ABI entries are exported and bound, the entry point's flags, its shard /
gather bookkeeping on 2 gloo ranks, the clip_results.json schema, and the per-clip initial draw's independence of the batch
split and the rank count."""
import ctypes as C
import json
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("paa_model_fwd_bwd_rows", "paa_model_forward_rows", "paa_project_rows", "paa_compose_clamp_rows")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from paa_amd import _lib
    return _lib


def test_new_entries_declared_exported_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "paa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(paa_[a-z0-9_]+)\s*\(", hdr))
    L = lib.lib()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in lib.exported_symbols(), name
        assert hasattr(L, name), name
    assert L.paa_version() in lib.ABI_VERSIONS


def test_new_entries_validate_arguments_without_gpu(lib):
    """Argument checks run on the host before any launch."""
    from paa_amd import runtime
    from paa_amd.training_utils import parser
    args = parser.create_arg_parser().parse_args(["--norm_type", "snr"])
    prm = runtime.params_of(args)
    L = lib.lib()
    assert L.paa_project_rows(None, C.byref(prm), None, None, 2, None, 16000, None) == lib.PAA_ERR_ARG
    assert L.paa_compose_clamp_rows(None, None, 2, None, 2, 16000, None) == lib.PAA_ERR_ARG
    assert L.paa_model_fwd_bwd_rows(None, None, None, 2, None, 2, 1, 1, None, None, None, None) == lib.PAA_ERR_ARG
    assert L.paa_model_forward_rows(None, None, None, 2, 1, None, 2, 1, None, None, None) == lib.PAA_ERR_ARG
    dummy = C.c_void_p(16)        # never dereferenced: the row count is refused first
    assert L.paa_compose_clamp_rows(dummy, dummy, 3, dummy, 2, 16000, None) == lib.PAA_ERR_SIZE


def test_parser_new_flags_and_defaults():
    from paa_amd import attack_clips
    a = attack_clips.create_arg_parser().parse_args([])
    assert a.pgd_steps == 100 and a.split == "test"
    assert a.norm_type == "max_phon" and a.batch_size == 64          # the runner's flags, unchanged
    a = attack_clips.create_arg_parser().parse_args(["--pgd_steps", "20", "--split", "val", "--norm_type", "snr"])
    assert a.pgd_steps == 20 and a.split == "val" and a.norm_type == "snr"
    with pytest.raises(SystemExit):
        attack_clips.create_arg_parser().parse_args(["--split", "dev"])


def _batches(n, bs, L=8):
    x = torch.arange(n * L, dtype=torch.float32).view(n, L)
    texts = [f"clip {i}" for i in range(n)]
    return [(x[i:i + bs], texts[i:i + bs]) for i in range(0, n, bs)]


def test_clip_batches_indices_cover_the_split():
    from paa_amd.attack_clips import clip_batches
    one = clip_batches(_batches(7, 3))
    assert [i for _, _, idx in one for i in idx] == list(range(7))
    for x, texts, idx in one:
        assert [t for t in texts] == [f"clip {i}" for i in idx]
        assert torch.equal(x[:, 0], torch.tensor([8.0 * i for i in idx]))
    # two ranks over global batches of 2 * 3 clips: disjoint shards, together the whole split, rows still match the indices
    got = []
    for r in range(2):
        for x, texts, idx in clip_batches(_batches(7, 6), r, 2):
            assert torch.equal(x[:, 0], torch.tensor([8.0 * i for i in idx]))
            got += idx
    assert sorted(got) == list(range(7)) and len(got) == 7


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from paa_amd import attack_clips as AC
    dist.init_process_group("gloo", rank=rank, world_size=world)
    recs = []
    for x, texts, idx in AC.clip_batches(_batches(9, 2 * world), rank, world):
        recs += [{"index": i, "clean_wer": 0.0, "adv_wer": 1.0, "clean_ctc": 1.0, "final_ctc": float(x[b, 0]), "l2": 0.5,
                  "linf": 0.1, "snr_db": 40.0} for b, i in enumerate(idx)]
    recs = AC.gather_records(recs, world)
    if rank == 0:
        args = types.SimpleNamespace(norm_type="snr", attack_mode="untargeted", optimizer_type="pgd", split="test", pgd_steps=3)
        AC.write_results(os.path.join(out_dir, "clip_results.json"), recs, args)
    dist.barrier()
    dist.destroy_process_group()


def test_shard_and_gather_on_two_gloo_ranks(tmp_path):
    from paa_amd import attack_clips as AC
    ctx = mp.get_context("spawn")
    port = _free_port()
    ps = [ctx.Process(target=_gather_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    got = json.load(open(tmp_path / "clip_results.json"))
    assert [r["index"] for r in got["clips"]] == list(range(9))
    assert [r["final_ctc"] for r in got["clips"]] == [8.0 * i for i in range(9)]      # each record kept its own clip's row
    # the same records as one rank computes them
    one = []
    for x, texts, idx in AC.clip_batches(_batches(9, 2)):
        one += [float(x[b, 0]) for b in range(len(idx))]
    assert one == [r["final_ctc"] for r in got["clips"]]
    assert got["summary"]["clips"] == 9


def test_results_schema():
    from paa_amd import attack_clips as AC
    recs = [{"index": i, "clean_wer": 0.0, "adv_wer": 0.5 * i, "clean_ctc": 2.0, "final_ctc": 3.0 + i, "l2": 0.1, "linf": 0.01,
             "snr_db": 40.0, "target_wer": 1.0} for i in range(3)]
    args = types.SimpleNamespace(norm_type="max_phon", attack_mode="targeted", optimizer_type="adam", split="val", pgd_steps=5)
    d = AC.results_dict(recs, args)
    assert set(d) == {"norm_type", "attack_mode", "optimizer_type", "split", "pgd_steps", "clips", "summary"}
    for r in d["clips"]:
        assert set(AC.RECORD_FIELDS) <= set(r) and AC.TARGET_FIELD in r
    s = d["summary"]
    assert s["clips"] == 3 and abs(s["adv_wer"] - 0.5) < 1e-12 and abs(s["final_ctc"] - 4.0) < 1e-12
    assert set(AC.SUMMARY_FIELDS) | {AC.TARGET_FIELD, "clips"} == set(s)
    json.dumps(d)
    args.attack_mode = "untargeted"
    assert AC.TARGET_FIELD not in AC.results_dict(recs, args)["summary"]


def test_per_clip_init_independent_of_split_and_ranks():
    from paa_amd.attack_clips import clip_batches
    from paa_amd.training_utils.clip_attack import init_rows
    L = 4000
    whole = init_rows(L, range(7), seed=5)
    assert whole.shape == (7, L) and whole.dtype == np.float32
    assert not np.array_equal(whole[0], whole[1])
    for bs, world in ((3, 1), (2, 2), (1, 3), (7, 2)):
        for r in range(world):
            for _, _, idx in clip_batches(_batches(7, bs * world), r, world):
                assert np.array_equal(init_rows(L, idx, seed=5), whole[idx])
    assert not np.array_equal(init_rows(L, [0], seed=6)[0], whole[0])


def test_params_of_norm_override_equals_a_cloned_namespace():
    """``params_of(args, n)`` is, field for field, what ``params_of`` gives for a copy of ``args`` whose norm_type is ``n``."""
    import copy
    from paa_amd import _lib, runtime
    from paa_amd.training_utils import parser
    args = parser.create_arg_parser().parse_args(["--norm_type", "linf+tv+masking", "--linf_size", "0.02", "--tv_epsilon", "0.5",
                                                  "--masking_margin_db", "-3", "--attack_mode", "targeted", "--lr", "3e-4"])
    for a in (args, types.SimpleNamespace(norm_type="snr+l2")):                   # the second: every field from its default
        for n in (*str(a.norm_type).split("+"), "masking"):
            clone = copy.copy(a)
            clone.norm_type = n
            want, got = runtime.params_of(clone), runtime.params_of(a, n)
            for field, _ in _lib.PaaParams._fields_:
                assert getattr(got, field) == getattr(want, field), (n, field)
        with pytest.raises(ValueError, match="Unknown norm_type"):
            runtime.params_of(a)                                                  # a '+'-joined list is no norm
        with pytest.raises(ValueError, match="Unknown norm_type"):
            runtime.params_of(a, "l3")


def test_clip_stepper_has_no_universal_surface():
    """Placement, the clip base of the draw and the host WER counters of the collective belong to the universal step alone."""
    from paa_amd.training_utils.clip_attack import ClipStepper
    from paa_amd.training_utils.pgd import PgdStepper
    for name in ("set_placement", "set_place_step", "clip_base", "set_wer_counts"):
        assert hasattr(PgdStepper, name), name
        assert not hasattr(ClipStepper, name), name
