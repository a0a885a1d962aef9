"""-m gpu: the library calls of one step, in order, for every mode of the universal and the per-clip stepper: what each mode adds
to the plain sequence and where, that a mode left off adds nothing, and that the sequence capture() puts into the graph is the
eager one.  The lists were recorded from the steppers as they were before they were given one shared core; the collective form is
recorded in tests/rccl_child.py."""
import numpy as np
import pytest
import torch

from gpu_util import record_launches

pytestmark = pytest.mark.gpu
B, L = 3, 8000
TEXTS = ["ab cd", "hello", "a b c"]
PLACE = ["--perturbation_seconds", "0.25", "--place_shift", "random", "--place_gain_db", "3"]
WER = ["paa_argmax_ids", "paa_wer_counts"]
# name: (per-clip, flags, device_wer, sequence)
CASES = {
    "universal pgd snr": (False, ["--optimizer_type", "pgd", "--norm_type", "snr"], False,
                          ["paa_model_fwd_bwd", "paa_sign_step", "paa_project"]),
    "universal adam linf+tv": (False, ["--optimizer_type", "adam", "--norm_type", "linf+tv"], False,
                               ["paa_model_fwd_bwd", "paa_adam_step", "paa_project", "paa_project"]),
    "universal pgd linf alpha": (False, ["--optimizer_type", "pgd", "--norm_type", "linf", "--masking_loss_alpha", "1e-6"], False,
                                 ["paa_model_fwd_bwd", "paa_masking_loss", "paa_sign_step", "paa_project"]),
    "universal pgd snr device_wer": (False, ["--optimizer_type", "pgd", "--norm_type", "snr"], True,
                                     ["paa_model_fwd_bwd", *WER, "paa_sign_step", "paa_project", "paa_stats_push"]),
    "universal pgd linf placement": (False, ["--optimizer_type", "pgd", "--norm_type", "linf", *PLACE], False,
                                     ["paa_place_draw", "paa_place_rows", "paa_model_fwd_bwd_rows", "paa_place_reduce",
                                      "paa_sign_step", "paa_project"]),
    "per-clip pgd snr": (True, ["--optimizer_type", "pgd", "--norm_type", "snr"], False,
                         ["paa_model_fwd_bwd_rows", "paa_sign_step", "paa_project_rows"]),
    "per-clip adam linf alpha device_wer": (True, ["--optimizer_type", "adam", "--norm_type", "linf", "--masking_loss_alpha", "1e-6"],
                                            True, ["paa_model_fwd_bwd_rows", "paa_masking_loss", *WER, "paa_adam_step",
                                                   "paa_project_rows", "paa_stats_push"]),
}


def make(name):
    """(stepper, p, clean, labels, step keywords) of a case: tiny arch, fp32, B = 3, L = 8000."""
    from paa_amd import arch as A, runtime, synth
    from paa_amd.core import loss_helpers as LH
    from paa_amd.model import PaaModel
    from paa_amd.training_utils import parser, place
    from paa_amd.training_utils.clip_attack import ClipStepper
    from paa_amd.training_utils.pgd import PgdStepper
    per_clip, flags, device_wer, _ = CASES[name]
    args = parser.create_arg_parser().parse_args(["--arch", "tiny", "--dtype", "fp32", "--silent", "--lr", "1e-3", "--snr_db", "40",
                                                  "--linf_size", "0.01", *flags])
    args.device = "cuda"
    a = A.tiny()
    m = PaaModel(a, A.rule_weights(a), B, L, "fp32")
    clean = torch.from_numpy(synth.clean_audio(B, L)).cuda()
    labels = LH.make_labels(TEXTS, None, args, B)
    if per_clip:
        p = np.stack([synth.normal(synth.key_of(f"d{b}", 5), L) for b in range(B)]).astype(np.float32)
    else:
        p = synth.perturbation(place.perturbation_length(args, L)).reshape(1, -1)
    p = torch.from_numpy(p * np.float32(1e-2)).cuda()
    opt = None
    if args.optimizer_type == "adam":
        p = torch.nn.Parameter(p)
        opt = torch.optim.Adam([p], lr=args.lr)
    # The projection contexts are cached per process and grow on demand (the masking loss wants one bound per clip): at B rows
    # from the start, the first step creates none, whichever tests ran before this one.
    runtime.get_proj(args, "cuda", B, L)
    st = (ClipStepper if per_clip else PgdStepper)(m, args, L, optimizer=opt, device_wer=device_wer)
    return st, p, clean, labels, ({"refs": LH.encode_refs(TEXTS)} if device_wer else {})


def _eager_and_captured(st, p, clean, labels, kw, want):
    with record_launches() as eager:
        st.step(p.data, clean, labels, **kw)
    print("eager", eager)
    assert eager == want
    with record_launches() as cap:
        g, _ = st.capture(p.data, clean, labels, **kw)
    print("capture", cap)
    assert cap[:len(want)] == want                                  # the warm-up step
    assert cap[len(want):] == want                                  # the launches inside the graph
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence(name):
    st, p, clean, labels, kw = make(name)
    want = CASES[name][3]
    if "alpha" in name and "universal" in name:                     # alpha = 0 launches nothing; the switch needs no new stepper
        with record_launches() as on:
            st.step(p.data, clean, labels, **kw)
        assert on == want
        st.set_masking_alpha(0.0)
        with record_launches() as off:
            st.step(p.data, clean, labels, **kw)
        print("alpha 0", off)
        assert off == [n for n in want if n != "paa_masking_loss"]
        st.set_masking_alpha(1e-6)
    _eager_and_captured(st, p, clean, labels, kw, want)
    if "placement" in name:                                         # explicit shifts and gains: the draw is skipped
        st.set_placement([0, 5, 1999], [1.0, 0.5, 2.0])
        _eager_and_captured(st, p, clean, labels, kw, [n for n in want if n != "paa_place_draw"])
