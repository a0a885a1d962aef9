"""Which modes of the PGD step are on and which may run together: decided here and nowhere else.  ``Modes.of(args)``
reads every mode flag once; ``RULES`` is the table of refusals: the mode a rule belongs to, its condition over (modes, context), the
exception and its message.  ``check`` walks the rules it is given and raises the first that applies; the order of a walk, and of the
walks of an entry point, decides which refusal wins."""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass, replace  # noqa: F401  (replace: how a caller forces a mode on)

GAIN_DB_MAX = 20.0
DRIFT_PPM_MAX = 100000.0
NOISE_SNR_MIN, NOISE_SNR_MAX = -20.0, 100.0
EOT_DRAWS_MAX = 64
MASK_LAGS_MAX = 32            # lags a table of paa_proj_set_masking_spread holds
MASK_DECAY_DB, MASK_RANGE_DB = 60.0, 96.0


def _pair(v):
    """--noise_snr_db as a tuple (of floats where they are numbers); None stays None; anything else is kept for "chan_range"."""
    if v is None:
        return None
    try:
        return tuple(float(x) if isinstance(x, (int, float, str)) else x for x in v)
    except (TypeError, ValueError):
        return (v,)


def _chan_bad(m):
    """None, or the first channel flag out of range."""
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and v == v
    if not (num(m.drift_ppm) and 0.0 <= m.drift_ppm <= DRIFT_PPM_MAX):
        return f"drift_ppm must be in [0, {DRIFT_PPM_MAX:g}], got {m.drift_ppm}"
    s = m.noise_snr
    if s is not None and not (len(s) == 2 and num(s[0]) and num(s[1]) and NOISE_SNR_MIN <= s[0] <= s[1] <= NOISE_SNR_MAX):
        return f"noise_snr_db must be LO HI with {NOISE_SNR_MIN:g} <= LO <= HI <= {NOISE_SNR_MAX:g} dB, got {list(s)}"
    return None


def mask_time_lags(ms, hop, sr):
    """J of temporal masking: the largest lag j in frames whose decrement j 60 hop 1000 / (ms sr) dB stays under the
    model's 96 dB range, counted up to MASK_LAGS_MAX + 1 (enough to refuse).  The products are taken in double in this written order."""
    j = 0
    while j <= MASK_LAGS_MAX and (j + 1) * MASK_DECAY_DB * hop * 1000.0 < MASK_RANGE_DB * ms * sr:
        j += 1
    return j


def mask_time_decrement(j, ms, hop, sr):
    """w[j] in dB, in double."""
    return j * MASK_DECAY_DB * hop * 1000.0 / (ms * sr)


def _mask_time_bad(m):
    """None, or the first of --masking_post_ms / --masking_pre_ms out of range."""
    for flag, v in (("masking_post_ms", m.post_ms), ("masking_pre_ms", m.pre_ms)):
        ok = isinstance(v, (int, float)) and not isinstance(v, bool) and 0.0 <= v < float("inf")
        if ok and (v == 0 or 1 <= mask_time_lags(v, m.hop, m.sr) <= MASK_LAGS_MAX):
            continue
        unit = 1000.0 * MASK_DECAY_DB / MASK_RANGE_DB * m.hop / m.sr          # the time whose decrement per frame is the whole range
        return (f"{flag} must be 0 (off) or lie in ({unit:g}, {unit * (MASK_LAGS_MAX + 1):g}] ms at hop_length {m.hop} and sr {m.sr} "
                f"(1 to {MASK_LAGS_MAX} frames of decay), got {v}")
    return None


@dataclass(frozen=True)
class Modes:
    norms: tuple                   # --norm_type, '+'-separated, in the written order
    masking_norm: bool
    alpha: float                   # --masking_loss_alpha
    place_on: bool                 # perturbation_seconds set, place_shift == "random" or place_gain_db > 0
    place_shift: str
    gain_db: float
    rir_on: bool                   # rir_bank other than "none"
    lengths_on: bool               # --clip_lengths true
    device_wer: bool
    optimizer_type: str
    drift_ppm: float = 0.0         # --drift_ppm
    noise_snr: tuple = None        # --noise_snr_db (LO, HI), or None
    loss_type: str = "ctc"         # --loss_type: "ctc", "margin" (the alignment-margin loss) or "feature" (§6q)
    kappa: float = 1.0             # --margin_kappa, in logits
    targeted: bool = False         # --attack_mode targeted
    eot_draws: int = 0             # --eot_draws G (attack_clips only): draws of the playback chain per clip, 0 = off
    seconds_on: bool = False       # --perturbation_seconds set
    anneal_on: bool = False        # --alpha_search other than "off" (attack_clips only)
    post_ms: float = 0.0           # --masking_post_ms (temporal masking), 0 = off
    pre_ms: float = 0.0            # --masking_pre_ms
    hop: int = 256                 # --hop_length and --sr: the frame period the two times are counted in
    sr: int = 16000
    search_on: bool = False        # --bound_search other than "off" (attack_clips only)

    @classmethod
    def of(cls, args=None, **flags):
        """The record of ``args`` (any object; a missing flag is off), ``flags`` overriding."""
        get = lambda k, d: flags.get(k, getattr(args, k, d))
        _num = lambda v: float(v) if isinstance(v, (int, float, str)) else v      # no number: kept, and raises where it is compared
        norms = tuple(str(get("norm_type", "")).split("+"))
        shift, gain, alpha = get("place_shift", "none"), _num(get("place_gain_db", 0.0)), _num(get("masking_loss_alpha", 0.0) or 0.0)
        on = get("perturbation_seconds", None) is not None or shift == "random" or (isinstance(gain, float) and gain > 0)
        return cls(norms, "masking" in norms, alpha, on, shift, gain, str(get("rir_bank", "none")) != "none",
                   str(get("clip_lengths", "padded")) == "true", bool(get("device_wer", False)), get("optimizer_type", None),
                   drift_ppm=_num(get("drift_ppm", 0.0) or 0.0), noise_snr=_pair(get("noise_snr_db", None)),
                   search_on=str(get("bound_search", "off")) != "off", anneal_on=str(get("alpha_search", "off")) != "off", loss_type=str(get("loss_type", "ctc")),
                   kappa=_num(get("margin_kappa", 1.0)), targeted=str(get("attack_mode", "untargeted")) == "targeted",
                   eot_draws=get("eot_draws", 0) or 0, seconds_on=get("perturbation_seconds", None) is not None,
                   post_ms=_num(get("masking_post_ms", 0.0) or 0.0), pre_ms=_num(get("masking_pre_ms", 0.0) or 0.0),
                   hop=int(get("hop_length", 256)), sr=int(get("sr", 16000)))

    drift_on = property(lambda m: isinstance(m.drift_ppm, float) and m.drift_ppm > 0)
    noise_on = property(lambda m: m.noise_snr is not None)
    chan_on = property(lambda m: m.drift_on or m.noise_on)        # the playback channel: clock drift and / or ambient noise
    shift_on = property(lambda m: m.place_shift == "random")
    masking = property(lambda m: m.masking_norm or m.alpha > 0)      # either pairs delta's frames with the clean clip's
    chan_why = property(lambda m: _chan_bad(m))
    margin_on = property(lambda m: m.loss_type == "margin")
    feature_on = property(lambda m: m.loss_type == "feature")          # the label-free feature-distance loss
    eot_on = property(lambda m: isinstance(m.eot_draws, int) and not isinstance(m.eot_draws, bool) and m.eot_draws >= 1)
    link_on = property(lambda m: m.place_on or m.rir_on or m.chan_on)      # at least one link of the playback chain
    mask_time_on = property(lambda m: any(isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0 for v in (m.post_ms, m.pre_ms)))
    mask_time_why = property(lambda m: _mask_time_bad(m))


SIZED_NORMS = ("l2", "linf", "snr", "tv", "fletcher_munson", "max_phon")      # the norms a bound scale tightens (min_max_freqs has no size)


def _wer_milli(args):
    """--search_success_wer in thousandths (0: not a usable number)."""
    wer = getattr(args, "search_success_wer", 0.5)
    return int(round(float(wer) * 1000)) if isinstance(wer, (int, float)) and wer == wer and abs(wer) < 1e6 else 0


class SearchConfig(namedtuple("SearchConfig", "shrink floor_scale wer_milli targeted")):
    """The per-clip bound search: on success a clip's bound scale is multiplied by ``shrink`` down to ``floor_scale``;
    untargeted success is per-clip WER >= ``wer_milli`` / 1000, targeted success the target transcript exactly."""

    @classmethod
    def of(cls, args):
        """The flags of ``args`` as they are (the "search_range" rule judges them); None with the search off."""
        if str(getattr(args, "bound_search", "off")) == "off":
            return None
        return cls(getattr(args, "search_shrink", 0.8), getattr(args, "search_floor", 0.01), _wer_milli(args),
                   getattr(args, "attack_mode", "untargeted") == "targeted")

    def bad(self):
        """None, or the first value out of range."""
        num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
        if not (num(self.shrink) and 0.0 < self.shrink < 1.0):
            return f"search_shrink must lie in (0, 1), got {self.shrink}"
        if not (num(self.floor_scale) and 0.0 < self.floor_scale <= 1.0):
            return f"search_floor must lie in (0, 1], got {self.floor_scale}"
        if not (isinstance(self.wer_milli, int) and self.wer_milli >= 1):
            return "search_success_wer must be at least 0.0005 (it is rounded to thousandths)"
        return None


class AnnealConfig(namedtuple("AnnealConfig", "up down up_every down_every alpha_min alpha_max wer_milli targeted")):
    """The per-clip masking-loss weight schedule: on success a clip's alpha is multiplied by ``up`` every ``up_every``
    steps, on failure by ``down`` every ``down_every`` steps, clamped to [``alpha_min``, ``alpha_max``]; success as SearchConfig's."""

    @classmethod
    def of(cls, args):
        """The flags of ``args`` as they are (the "anneal_range" rule judges them); None with the schedule off.  A clamp that is not
        given derives from alpha0 = --masking_loss_alpha: alpha0 / 100 (Qin's floor) and alpha0 * 100."""
        if str(getattr(args, "alpha_search", "off")) == "off":
            return None
        a0 = getattr(args, "masking_loss_alpha", 0.0) or 0.0
        a0 = float(a0) if isinstance(a0, (int, float)) and not isinstance(a0, bool) else 0.0
        lo, hi = getattr(args, "alpha_min", None), getattr(args, "alpha_max", None)
        return cls(getattr(args, "alpha_up", 1.2), getattr(args, "alpha_down", 0.8), getattr(args, "alpha_up_every", 20),
                   getattr(args, "alpha_down_every", 50), a0 / 100.0 if lo is None else lo, a0 * 100.0 if hi is None else hi,
                   _wer_milli(args),
                   getattr(args, "attack_mode", "untargeted") == "targeted")

    def bad(self, alpha0=None):
        """None, or the first value out of range (the ranges of paa_clip_anneal; with ``alpha0``, the clamps must enclose it)."""
        num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
        period = lambda v: isinstance(v, int) and not isinstance(v, bool) and v >= 1
        if not (num(self.up) and 1.0 < self.up < float("inf")):
            return f"alpha_up must be finite and > 1, got {self.up}"
        if not (num(self.down) and 0.0 < self.down < 1.0):
            return f"alpha_down must lie in (0, 1), got {self.down}"
        if not period(self.up_every):
            return f"alpha_up_every must be an integer >= 1, got {self.up_every}"
        if not period(self.down_every):
            return f"alpha_down_every must be an integer >= 1, got {self.down_every}"
        if not (num(self.alpha_min) and num(self.alpha_max) and 0.0 < self.alpha_min <= self.alpha_max < float("inf")):
            return f"need 0 < alpha_min <= alpha_max < inf, got alpha_min {self.alpha_min}, alpha_max {self.alpha_max}"
        if not (isinstance(self.wer_milli, int) and self.wer_milli >= 1):
            return "search_success_wer must be at least 0.0005 (it is rounded to thousandths)"
        if alpha0 is not None and not self.alpha_min <= alpha0 <= self.alpha_max:
            return (f"the clamps must enclose the starting weight: alpha_min {self.alpha_min} <= masking_loss_alpha {alpha0} <= "
                    f"alpha_max {self.alpha_max}")
        return None


# eager_adam: torch's own optimizer.step() runs the update, not the device step; L / Lp: clip / perturbation length, where known;
# search: the SearchConfig of the run; wer_why: why the device WER route is not available (None: it is); anneal: the AnnealConfig of
# the run; alpha0: the weight the schedule starts from; stage1 / steps: --stage1_steps as given (None: not given) and --pgd_steps
class Ctx(namedtuple("Ctx", "world eager_adam L Lp search wer_why anneal alpha0 stage1 steps",
                     defaults=(1, False, None, None, None, None, None, None, None, None))):
    __slots__ = ()
    search_why = property(lambda c: "bound search is on without a SearchConfig" if c.search is None else c.search.bad())
    anneal_why = property(lambda c: "alpha search is on without an AnnealConfig" if c.anneal is None else c.anneal.bad(c.alpha0))
    stage1_steps = property(lambda c: stage1_of(c.stage1, c.steps))


def stage1_of(stage1, steps):
    """Steps of stage 1 in the two-stage run: --stage1_steps, or half of --pgd_steps."""
    return int(steps) // 2 if stage1 is None else stage1


def _stage_bad(m, c):
    both = m.search_on and m.anneal_on
    if not both:
        return c.stage1 is not None
    s = c.stage1_steps
    return not (isinstance(s, int) and not isinstance(s, bool) and 1 <= s <= int(c.steps) - 1)
# mode: the field of Modes that must be on for the rule to apply, or None; when(modes, ctx); msg: formatted with m = modes, c = ctx
Rule = namedtuple("Rule", "mode when exc msg")
_PAIRS = ": both pair the perturbation's frames with the clean clip's frames"
_DEVICE_STEP = " the device step: use the defaults of torch.optim.Adam(lr=...) or --optimizer_type pgd"
_NO_LEN = "--clip_lengths true does not support "
_SEARCH = "--bound_search shrink "
_ANNEAL = "--alpha_search qin "
_UNIVERSAL = "the universal perturbation (paa_amd.run_attack); per-clip perturbations have no "
NIE = NotImplementedError
RULES = {
    "route": Rule("masking_norm", lambda m, c: c.world > 1, NIE, "the masking norm is not implemented for data-parallel universal "
                  "perturbations (world size {c.world}): the bound would need a MIN-reduction across ranks; use one rank, or per-clip "
                  "perturbations (paa_amd.attack_clips)"),
    "alpha_range": Rule(None, lambda m, c: m.alpha < 0, ValueError, "masking_loss_alpha must be >= 0, got {m.alpha}"),
    "alpha_eager": Rule(None, lambda m, c: c.eager_adam and m.alpha > 0, NIE, "masking_loss_alpha > 0 needs" + _DEVICE_STEP),
    # placement
    "shift_range": Rule("place_on", lambda m, c: m.place_shift not in ("none", "random"), ValueError,
                        "place_shift must be 'none' or 'random', got {m.place_shift!r}"),
    "gain_range": Rule("place_on", lambda m, c: not 0.0 <= m.gain_db <= GAIN_DB_MAX, ValueError,
                       f"place_gain_db must be in [0, {GAIN_DB_MAX:g}], got {{m.gain_db}}"),
    "place_masking": Rule("place_on", lambda m, c: m.masking, NIE, "placement (perturbation_seconds / place_shift / place_gain_db) is "
                          "not implemented with the masking norm or masking_loss_alpha > 0" + _PAIRS),
    "place_snr_tv": Rule("place_on", lambda m, c: c.Lp != c.L and any(n in ("snr", "tv") for n in m.norms), NIE,
                         "the snr / tv norms need a perturbation as long as the clips (Lp = {c.Lp}, L = {c.L}): their bound "
                         "compares the two sample for sample"),
    "place_eager": Rule("place_on", lambda m, c: c.eager_adam, NIE, "placement needs" + _DEVICE_STEP),
    "place_clips": Rule("place_on", lambda m, c: True, NIE,
                        "--perturbation_seconds / --place_shift / --place_gain_db apply to " + _UNIVERSAL + "placement"),
    # room responses
    "rir_masking": Rule("rir_on", lambda m, c: m.masking, NIE,
                        "room responses (rir_bank) are not implemented with the masking norm or masking_loss_alpha > 0" + _PAIRS),
    "rir_eager": Rule("rir_on", lambda m, c: c.eager_adam, NIE, "room responses (rir_bank) need" + _DEVICE_STEP),
    "rir_clips": Rule("rir_on", lambda m, c: True, NIE, "--rir_bank applies to " + _UNIVERSAL + "room responses yet"),
    # the playback channel: clock drift and ambient noise
    "chan_range": Rule(None, lambda m, c: _chan_bad(m) is not None, ValueError, "{m.chan_why}"),
    "chan_masking": Rule("chan_on", lambda m, c: m.masking, NIE, "the playback channel (drift_ppm / noise_snr_db) is not "
                         "implemented with the masking norm or masking_loss_alpha > 0" + _PAIRS),
    "chan_eager": Rule("chan_on", lambda m, c: c.eager_adam, NIE, "the playback channel (drift_ppm / noise_snr_db) needs" + _DEVICE_STEP),
    "chan_clips": Rule("chan_on", lambda m, c: True, NIE,
                       "--drift_ppm / --noise_snr_db apply to " + _UNIVERSAL + "playback channel yet"),
    # true clip lengths: each of these needs a design of its own before it may meet them
    "len_masking": Rule("lengths_on", lambda m, c: m.masking_norm, ValueError, _NO_LEN + "--norm_type masking"),
    "len_alpha": Rule("lengths_on", lambda m, c: m.alpha > 0, ValueError, _NO_LEN + "--masking_loss_alpha > 0"),
    "len_place": Rule("lengths_on", lambda m, c: m.place_on, ValueError,
                      _NO_LEN + "placement (--perturbation_seconds, --place_shift, --place_gain_db)"),
    "len_rir": Rule("lengths_on", lambda m, c: m.rir_on, ValueError, _NO_LEN + "--rir_bank"),
    "len_chan": Rule("lengths_on", lambda m, c: m.chan_on, ValueError, _NO_LEN + "--drift_ppm / --noise_snr_db"),
    "len_eager": Rule("lengths_on", lambda m, c: c.eager_adam, NIE, "--clip_lengths true needs" + _DEVICE_STEP),
    # per-clip bound search
    "search_range": Rule("search_on", lambda m, c: c.search is None or c.search.bad() is not None, ValueError,
                         "{c.search_why}"),
    "search_masking": Rule("search_on", lambda m, c: m.masking_norm, NIE, _SEARCH + "is not implemented with --norm_type masking: "
                           "a per-clip threshold with a moving margin is a change of its own"),
    "search_no_size": Rule("search_on", lambda m, c: not any(n in SIZED_NORMS for n in m.norms), ValueError,
                           _SEARCH + "needs a norm with a size to shrink; {m.norms} has none"),
    "search_route": Rule("search_on", lambda m, c: c.wer_why is not None, NIE,
                         _SEARCH + "decides success from the on-device WER counters, which are not available: {c.wer_why}"),
    # per-clip adaptive masking-loss weight
    "anneal_alpha0": Rule("anneal_on", lambda m, c: not m.alpha > 0, ValueError,
                          _ANNEAL + "needs --masking_loss_alpha > 0: that value is the weight every clip starts from"),
    "anneal_range": Rule("anneal_on", lambda m, c: c.anneal is None or c.anneal.bad(c.alpha0) is not None,
                         ValueError, "{c.anneal_why}"),
    "anneal_stage": Rule(None, lambda m, c: c.steps is not None and _stage_bad(m, c), ValueError,
                         "--stage1_steps applies to the two-stage run (--bound_search shrink with --alpha_search qin) and must lie in "
                         "[1, pgd_steps - 1]: got stage1_steps {c.stage1_steps} with pgd_steps {c.steps}, bound search "
                         "{m.search_on}, alpha search {m.anneal_on}"),
    "anneal_route": Rule("anneal_on", lambda m, c: c.wer_why is not None, NIE,
                         _ANNEAL + "decides success from the on-device WER counters, which are not available: {c.wer_why}"),
    # the alignment-margin loss
    "margin_untargeted": Rule("margin_on", lambda m, c: not m.targeted, ValueError,
                              "--loss_type margin needs --attack_mode targeted: the hinge is flat wherever the aligned class already "
                              "wins, so it is no untargeted objective"),
    "margin_kappa": Rule("margin_on", lambda m, c: not (isinstance(m.kappa, (int, float)) and not isinstance(m.kappa, bool)
                                                        and 0.0 <= m.kappa < float("inf")), ValueError,
                         "margin_kappa must be finite and >= 0, got {m.kappa}"),
    # temporal masking of the threshold
    "mask_time_range": Rule(None, lambda m, c: _mask_time_bad(m) is not None, ValueError, "{m.mask_time_why}"),
    "mask_time_unused": Rule("mask_time_on", lambda m, c: not m.masking, ValueError,
                             "--masking_post_ms / --masking_pre_ms spread the masking threshold along time and need a consumer of it: "
                             "--norm_type masking or --masking_loss_alpha > 0"),
    # the feature-distance loss
    "feature_targeted": Rule("feature_on", lambda m, c: m.targeted, ValueError,
                             "--loss_type feature does not run with --attack_mode targeted: that mode names a target phrase, not a "
                             "target recording; targeted feature matching is available through the API (PaaModel.set_feature_loss "
                             "with any reference and direction = -1)"),
    "feature_eot": Rule("feature_on", lambda m, c: m.eot_on, NIE,
                        "--loss_type feature is not implemented with --eot_draws: the model's rows are then draws of the playback "
                        "chain on a zero clean operand, and the clean reference would need a chain of its own"),
    # per-clip perturbations through the playback chain
    "eot_range": Rule(None, lambda m, c: not (isinstance(m.eot_draws, int) and not isinstance(m.eot_draws, bool)
                                              and 0 <= m.eot_draws <= EOT_DRAWS_MAX), ValueError,
                      f"eot_draws must be an integer in [0, {EOT_DRAWS_MAX}], got {{m.eot_draws}}"),
    "eot_links": Rule("eot_on", lambda m, c: not m.link_on, ValueError,
                      "--eot_draws needs at least one link of the playback chain (--place_gain_db, --rir_bank, --drift_ppm, "
                      "--noise_snr_db): without one all draws of a clip are equal"),
    "eot_shift": Rule("eot_on", lambda m, c: m.shift_on or m.seconds_on, NIE,
                      "--eot_draws does not run with --place_shift random or --perturbation_seconds: a per-clip perturbation is "
                      "as long as its clip and has no position of its own"),
}

PLACE_FLAGS = ("shift_range", "gain_range", "place_masking")
PLACE = PLACE_FLAGS + ("place_snr_tv", "place_eager")
ROOMS = ("rir_masking", "rir_eager")
CHANNEL_FLAGS = ("chan_range", "chan_masking")
CHANNEL = CHANNEL_FLAGS + ("chan_eager",)
LENGTHS = ("len_masking", "len_alpha", "len_place", "len_rir", "len_chan")
SEARCH_FLAGS = ("search_range", "search_masking", "search_no_size")       # known from the flags alone
MARGIN = ("margin_untargeted", "margin_kappa")                            # known from the flags alone
FEATURE = ("feature_targeted", "feature_eot")                             # known from the flags alone
EOT = ("eot_range", "eot_links", "eot_shift")                              # known from the flags alone
MASK_TIME = ("mask_time_range", "mask_time_unused")                        # known from the flags alone
SEARCH = SEARCH_FLAGS + ("search_route",)                                  # ... and once the vocabulary and the references are known


ANNEAL_FLAGS = ("anneal_alpha0", "anneal_range", "anneal_stage")           # known from the flags alone
ANNEAL = ANNEAL_FLAGS + ("anneal_route",)                                  # ... and once the vocabulary and the references are known


def anneal_ctx(args, **kw):
    """The context the schedule's rules read, from the flags of ``args``."""
    a0 = Modes.of(args).alpha
    return Ctx(search=SearchConfig.of(args), anneal=AnnealConfig.of(args), alpha0=a0 if isinstance(a0, float) else None,
               stage1=getattr(args, "stage1_steps", None), steps=getattr(args, "pgd_steps", None), **kw)


def check(m: Modes, keys, c: Ctx = Ctx()) -> Modes:
    """Raises the first of the rules ``keys`` that applies; returns ``m``."""
    for r in map(RULES.get, keys):
        if (r.mode is None or getattr(m, r.mode)) and r.when(m, c):
            raise r.exc(r.msg.format(m=m, c=c))
    return m
