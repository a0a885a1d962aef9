"""Command-line surface of the reference's ``src/training_utils/parser.py`` (same flags, types and
defaults — SURVEY §5.6) plus the non-breaking additions of SURVEY §8b."""
import argparse

NORM_CHOICES = ["l2", "linf", "snr", "tv", "fletcher_munson", "min_max_freqs", "max_phon", "masking"]


def _norm_type(v: str) -> str:
    parts = v.split("+")
    for part in parts:
        if part not in NORM_CHOICES:
            raise argparse.ArgumentTypeError(f"invalid choice: {v!r} (choose from {NORM_CHOICES}, or 'a+b')")
    return v


def _place_gain_db(v: str) -> float:
    g = float(v)
    if not 0.0 <= g <= 20.0:
        raise argparse.ArgumentTypeError(f"place_gain_db must be in [0, 20], got {v}")
    return g


def _ranged(name, lo, hi, typ):
    def conv(v: str):
        x = typ(v)
        if not lo <= x <= hi:
            raise argparse.ArgumentTypeError(f"{name} must be in [{lo:g}, {hi:g}], got {v}")
        return x
    conv.__name__ = name
    return conv


def create_arg_parser():
    parser = argparse.ArgumentParser()
    # standard training params (parser.py:10-20)
    parser.add_argument('--batch_size', type=int, default=64, help='batch size')
    parser.add_argument('--lr', type=float, default=1e-4, help='lr for the perturbation update')
    parser.add_argument('--early_stopping', type=int, default=4, help='how many epochs to wait before early stopping')
    parser.add_argument('--num_epochs', type=int, default=50, help='how many epochs at all')
    parser.add_argument('--optimizer_type', type=str, choices=["adam", "pgd"], default='adam',
                        help='how to optimize the perturbation update')
    parser.add_argument('--gamma', type=float, default=0.9, help='weight decay')
    parser.add_argument('--step_size', type=int, default=2, help='how many epochs does it take before we decay weights')
    parser.add_argument('--dataset', type=str, default="LibreeSpeech", choices=["LibreeSpeech", "CommonVoice", "tedlium"])
    parser.add_argument('--resume_from', type=str, default=None,
                        help='Path to a saved perturbation .pt file to resume training from')
    # adversarial params (parser.py:29-53)
    parser.add_argument('--target_reps', type=int, default=5)
    parser.add_argument('--target', type=str, default="delete", help='Target phrase for targeted attacks')
    parser.add_argument('--attack_mode', type=str, choices=["untargeted", "targeted"], default="untargeted")
    parser.add_argument('--norm_type', type=_norm_type, default='max_phon',
                        help='type of norm to limit the perturbation (extension: "a+b" applies a then b)')
    parser.add_argument('--fm_epsilon', type=float, default=2)
    parser.add_argument('--l2_size', type=float, default=0.05)
    parser.add_argument('--linf_size', type=float, default=0.0001)
    parser.add_argument('--snr_db', type=float, default=64)
    parser.add_argument('--min_freq_attack', type=float, default=120)
    parser.add_argument('--max_freq_attack', type=float, default=20_000)
    parser.add_argument('--tv_epsilon', type=float, default=0.001)
    parser.add_argument('--max_phon_level', type=float, default=20)
    parser.add_argument('--masking_margin_db', type=float, default=0.0,
                        help='masking norm (extension): dB added to the clean clip\'s masking threshold')
    parser.add_argument('--masking_loss_alpha', type=float, default=0.0,
                        help='masking-threshold loss term (extension): the step optimises direction * CTC - alpha * sum_b l_b; '
                             '0 = off')
    # temporal masking (extension); the defaults leave every threshold as it is.  Documented example: 200 / 20
    parser.add_argument('--masking_post_ms', type=float, default=0.0,
                        help='post-masking: a frame\'s masking threshold lasts on after it, falling by 60 dB over this many ms; 0 = off')
    parser.add_argument('--masking_pre_ms', type=float, default=0.0,
                        help='pre-masking: a frame\'s masking threshold reaches back before it, falling by 60 dB over this many ms; 0 = off')
    # sound properties (parser.py:57-63)
    parser.add_argument('--phon_reference_db', type=float, default=65)
    parser.add_argument('--sr', type=int, default=16000)
    parser.add_argument('--n_fft', type=int, default=1024)
    parser.add_argument('--hop_length', type=int, default=256)
    parser.add_argument('--win_length', type=int, default=1024)
    parser.add_argument('--relative_audio_length', type=float, default=0.80)
    # others (parser.py:64-66)
    parser.add_argument('--seed', type=int, default=5)
    parser.add_argument('--small_data', action='store_true')
    parser.add_argument('--num_items_to_inspect', type=int, default=12)
    # additions: none changes the meaning of a reference flag
    parser.add_argument('--device', type=str, default="cuda")
    parser.add_argument('--model_path', type=str, default=None, help='local HF checkpoint directory (no hub access)')
    parser.add_argument('--arch', type=str, choices=["base", "large-lv60", "tiny"], default="base",
                        help='architecture for rule-generated weights when no --model_path is given')
    parser.add_argument('--dtype', type=str, choices=["bf16", "fp32"], default="bf16",
                        help='MFMA operand precision: bf16, or fp32 = split-bf16 (3 passes), fp32-parity')
    parser.add_argument('--audio_seconds', type=float, default=10.0, help='clip length for synthetic data')
    parser.add_argument('--steps_per_epoch', type=int, default=4, help='synthetic batches per epoch')
    parser.add_argument('--data_dir', type=str, default=None, help='local directory of wav files + transcripts (no download)')
    parser.add_argument('--logs_dir', type=str, default=None, help='root of the run directories (default ./logs)')
    parser.add_argument('--silent', action='store_true')
    parser.add_argument('--device_wer', action='store_true',
                        help='count word errors on the device (greedy CTC decode + edit distance) and read the per-step scores back '
                             'once per epoch; single-character vocabularies without a wer_metric object, else the host path')
    # random placement of the universal perturbation (extension); the defaults leave the step as it is
    parser.add_argument('--perturbation_seconds', type=float, default=None,
                        help='length of the universal perturbation in seconds (default: the clip length); a shorter one is '
                             'tiled over the clip, a longer one windowed')
    parser.add_argument('--place_shift', type=str, choices=["none", "random"], default="none",
                        help='random: every clip of every step sees the perturbation at a circular shift of its own')
    parser.add_argument('--place_gain_db', type=_place_gain_db, default=0.0,
                        help='G in [0, 20]: every clip of every step sees the perturbation at a gain uniform in [-G, +G] dB')
    # true clip lengths (extension); the default leaves every object and file as it is
    parser.add_argument('--clip_lengths', type=str, choices=["padded", "true"], default="padded",
                        help='true: batches carry every clip\'s own sample count and the model masks the padding as HuggingFace does '
                             'with an attention_mask (compose, attention keys, CTC length, decode); padded: the padding is audio')
    # room responses on the placement layer (extension); the default leaves the step as it is
    parser.add_argument('--rir_bank', type=str, default="none",
                        help='none | synthetic | PATH (.npy or weights-only .pt holding a float (N, K) array): every clip of every '
                             'step hears the perturbation through a room response drawn from the bank')
    parser.add_argument('--rir_count', type=_ranged("rir_count", 1, 65536, int), default=64, help='responses in a synthetic bank')
    parser.add_argument('--rir_taps', type=_ranged("rir_taps", 1, 16384, int), default=4096, help='taps per response in a synthetic bank')
    parser.add_argument('--rir_rt60', type=_ranged("rir_rt60", 0.01, 10.0, float), nargs=2, default=[0.2, 0.6], metavar=("LO", "HI"),
                        help='RT60 range of a synthetic bank in seconds')
    parser.add_argument('--rir_drr_db', type=_ranged("rir_drr_db", -40.0, 60.0, float), default=6.0,
                        help='direct-to-reverberant energy ratio of a synthetic bank in dB')
    parser.add_argument('--rir_seed', type=int, default=None, help='seed of the synthetic bank (default: --seed)')
    # the playback channel on the placement layer (extension); the defaults leave the step as it is.  Both draw
    # under --place_seed / --seed, as the rooms do
    parser.add_argument('--drift_ppm', type=_ranged("drift_ppm", 0.0, 100000.0, float), default=0.0,
                        help='P in [0, 100000]: every clip of every step hears the perturbation resampled by a clock ratio uniform '
                             'in 1 +- P * 1e-6 (16-tap windowed sinc; no band-limiting, meant for P <= 100000); 0 = off')
    parser.add_argument('--noise_snr_db', type=_ranged("noise_snr_db", -20.0, 100.0, float), nargs=2, default=None,
                        metavar=("LO", "HI"), help='ambient noise: white Gaussian noise is added to every clip of every step at an '
                        'SNR uniform in [LO, HI] dB below the clean clip; absent = off')
    # the loss of the device step (extension); the default leaves the step as it is
    parser.add_argument('--loss_type', type=str, choices=["ctc", "margin", "feature"], default="ctc",
                        help='margin (targeted attacks only): the alignment-margin loss, a hinge on the frames where the forced '
                             'alignment of the target does not yet win the argmax by --margin_kappa; zero exactly when the greedy '
                             'decode is the target.  feature (untargeted attacks only): the label-free cosine distance between '
                             'the encoder\'s last hidden state of the perturbed clip and that of the clean clip')
    parser.add_argument('--margin_kappa', type=float, default=1.0, help='margin loss: the margin in logits, finite and >= 0')
    return parser
