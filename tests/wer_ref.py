"""NumPy restatement of ``paa_wer_counts`` (csrc/wer_kernels.hip): token ids -> canon table -> drop,
collapse on ids, words as code-point runs, Levenshtein rows by the prefix-min form the kernel's lanes run.  Works on integers only:
no strings, no tokenizer (``host_counts`` is the string path both are checked against).  tests/test_wer_host.py pins it to core/loss_helpers.py greedy_decode_ids + wer_texts + wer_counts;
tests/test_gpu_wer.py draws its cases from ``cases()`` too."""
import numpy as np

T_GRID = (1, 2, 7, 49, 499, 1499)


def kept_codes(ids, canon):
    """Drop the frames whose id maps to -1 FIRST, then keep a frame iff its id differs from the previous surviving id."""
    out, prev = [], None
    for i in ids:
        i = int(i)
        c = int(canon[i]) if 0 <= i < len(canon) else -1
        if c < 0:
            continue
        if i != prev:
            out.append(c)
        prev = i
    return out


def hyp_words(codes):
    """Maximal runs of non-delimiter code points (a leading / trailing delimiter yields no empty word)."""
    words, cur = [], []
    for c in codes:
        if c == 0:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(c)
    if cur:
        words.append(tuple(cur))
    return words


def ref_words(row):
    """A row ends at its first negative entry; every 0 before that terminates one word."""
    words, cur = [], []
    for c in row:
        c = int(c)
        if c < 0:
            break
        if c == 0:
            words.append(tuple(cur))
            cur = []
        else:
            cur.append(c)
    return words


def edit_distance_prefix_min(hyp, ref):
    """Unit-cost Levenshtein, one row per hypothesis word: t[j] = min(d_prev[j] + 1, d_prev[j - 1] + cost) and
    d[j] - j = min_{k <= j} (t[k] - k) with t[0] = d[0] = i — the scan the kernel does across lanes."""
    n = len(ref)
    d = np.arange(n + 1, dtype=np.int64)
    j = np.arange(n + 1, dtype=np.int64)
    for i, h in enumerate(hyp, 1):
        cost = np.array([0 if h == r else 1 for r in ref], dtype=np.int64)
        t = np.empty(n + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(d[1:] + 1, d[:-1] + cost)
        d = np.minimum.accumulate(t - j) + j
    return int(d[n])


def wer_counts_ref(ids, canon, refs):
    """ids (B, T) integer, canon (V) int32, refs (B, R) int32 -> (B, 3) int32 [errors, reference words, hypothesis words]."""
    ids, refs = np.asarray(ids), np.asarray(refs)
    out = np.zeros((ids.shape[0], 3), dtype=np.int32)
    for b in range(ids.shape[0]):
        h, r = hyp_words(kept_codes(ids[b], canon)), ref_words(refs[b])
        out[b] = (edit_distance_prefix_min(h, r), len(r), len(h))
    return out


def host_counts(ids, ref_text):
    """(errors, reference words, hypothesis words) of one clip by the string path of train_epoch / evaluate: greedy_decode_ids,
    the strip / lower of wer_texts, clean_transcripts on the reference, wer_counts."""
    from paa_amd.core import loss_helpers as LH
    pred = [p.strip().lower() for p in LH.greedy_decode_ids([list(map(int, ids))])]
    ref = [t.lower() for t in LH.clean_transcripts([ref_text])]
    e, w = LH.wer_counts(pred, ref)
    return e, w, len(pred[0].split())


# ---- seeded cases over the built-in 32-token vocabulary (ids 0..3 special, 4 = '|', 27 = "'") ------------------------------
LETTERS = [i for i in range(5, 32) if i != 27]
REF_POOL = ["", "a", "hello world", "it's a test", "the cat sat on the mat", "don't stop", "a <unk> b", "café naïve 123",
            "  spaced   out\ttext ", "<unk>", "x y z x y z x y z", "THE QUICK brown FOX", "ab cd", "rock'n'roll '' '"]


def _stream(kind, T, rng):
    if kind == "blank":
        return np.zeros(T, dtype=np.int64)
    if kind == "alternating":                       # letter / delimiter: the most words a stream can hold, ceil(T / 2)
        s = np.full(T, 4, dtype=np.int64)
        s[0::2] = rng.choice(LETTERS, size=len(s[0::2]))
        return s
    if kind == "specials_between":                  # A <pad> A, | <s> |, A <unk> B ...
        base = rng.choice([5, 5, 6, 4, 4, 27], size=T)
        sp = rng.random(T) < 0.4
        return np.where(sp, rng.integers(0, 4, size=T), base)
    if kind == "apostrophes":
        return rng.choice([27, 27, 4, 6, 12], size=T)
    if kind == "speechlike":                        # runs of repeated frames, blanks in between, words of a few letters
        out = []
        while len(out) < T:
            tok = int(rng.choice(LETTERS + [4, 4, 27, 0, 0, 0, 1, 3]))
            out += [tok] * int(rng.integers(1, 4))
        return np.array(out[:T], dtype=np.int64)
    return rng.integers(0, 32, size=T)              # "random"


KINDS = ("blank", "alternating", "specials_between", "apostrophes", "speechlike", "random")


def _decodable_ref(ids):
    """The text the stream itself decodes to (lower case), so that some cases have errors = 0 or a few edits."""
    from paa_amd.core import loss_helpers
    return loss_helpers.greedy_decode_ids([list(map(int, ids))])[0].lower()


def cases(seed=0, per_cell=4):
    """[(name, ids (T,), reference text)]: every kind at every T of T_GRID, ``per_cell`` seeded draws each, references from the
    pool, from the stream's own decode (exact and perturbed), empty, and with characters outside the vocabulary."""
    rng = np.random.default_rng(seed)
    out = []
    for T in T_GRID:
        for kind in KINDS:
            for n in range(per_cell):
                ids = _stream(kind, T, rng)
                pick = n % 4
                if pick == 0:
                    ref = REF_POOL[int(rng.integers(len(REF_POOL)))]
                elif pick == 1:
                    ref = _decodable_ref(ids)
                elif pick == 2:                     # the decode with words dropped / replaced / inserted
                    w = _decodable_ref(ids).split()
                    w = [x for x in w if rng.random() > 0.2]
                    w = [("zzé" if rng.random() < 0.1 else x) for x in w]
                    if w and rng.random() < 0.5:
                        w.insert(int(rng.integers(len(w))), "extra")
                    ref = " <unk> ".join(w[:3]) + " " + " ".join(w[3:])
                else:
                    ref = ""
                out.append((f"{kind}-T{T}-{n}", ids, ref))
    return out

