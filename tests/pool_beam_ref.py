"""numpy restatement of the pooled beam search's rule (include/univl_hip.h: univl_beam_pool_step, univl_beam_pool_finish), shared by
tests/test_pool_beam_cpu.py (identities of the reference itself, and the events its generator produces) and
tests/test_pool_beam_gpu.py (the kernels and the session bit for bit).  Written from the header's words in np.float32 arithmetic as
the plain thing: per instance ALL candidates are sorted and the list is walked.  It knows nothing of slices, per-row lists or a
separately read end column, so the kernel's sufficiency argument is tested, not assumed.  It shares no code with the package.

`events` collects what happened, by name, for the coverage checks."""
import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


def weights(alpha, Tmax):
    """w[L] = float32(float64(L) ** -alpha) for L = 1 .. Tmax + 1, w[0] = 1."""
    w = np.ones(Tmax + 2, dtype=np.float64)
    for L in range(1, Tmax + 2):
        w[L] = float(L) ** -float(alpha)
    return w.astype(F32)


def before(a, b):
    """Pool order on entries (key, raw, end_t, beam, finished): larger key, then smaller end_t, then smaller beam."""
    return a[0] > b[0] or (a[0] == b[0] and (a[2] < b[2] or (a[2] == b[2] and a[3] < b[3])))


def pool_sorted(pool):
    out = []
    for e in pool:                                            # insertion by the order itself (entries are distinct in (end_t, beam))
        k = 0
        while k < len(out) and not before(e, out[k]):
            k += 1
        out.insert(k, e)
    return out


EOS = 5
EVENTS = ("end_at_rank_nb_minus_1_taken", "end_at_rank_nb_not_taken", "all_rows_end_best", "end_at_t0", "replacement", "drop",
          "equal_key_by_end_t", "equal_key_by_beam", "done_by_bound", "done_by_early_stopping", "ran_to_Tmax_live_beams_pooled",
          "inf_end_not_pooled")
N_INST, TMAX = 3, 6
NBS, SHAPES, ALPHAS, MODES = (1, 3, 5, 8), ((37, 40, 0), (37, 40, 1), (30522, 30528, 0)), (0.0, 0.6, 2.0), (False, True)


def case_seed(nb, V, offset, alpha, early):
    return 1000 * nb + 100 * int(alpha * 5) + 10 * offset + (V % 7) + (50 if early else 0)


def make_lps(seed, nb, V, ld, Tmax=TMAX, n=N_INST):
    """The log-probabilities of one run, a list of Tmax arrays [n * nb, ld]: multiples of 1/4 (sums are exact, ties common), padding
    columns at +1e30 that must never win, the end column EOS far down except where it is raised:
      instance 0  from t = 1 on the end column is every row's best: the pool fills at once;
      instance 1  the end column is raised at t = 0 and, at later (position, row) pairs drawn at random, set EQUAL to one of the row's
                  top n_bm + 2 values, so that end candidates land on both sides of rank n_bm and tie with their neighbours;
      instance 2  the end column is -inf while t < 2 (a minimum length), then raised rarely: it usually runs to Tmax."""
    rng = np.random.RandomState(seed)
    lo = -max(60, V // 4)
    lps = []
    for t in range(Tmax):
        lp = (rng.randint(lo, -2, size=(n * nb, ld)) * 0.25).astype(F32)
        lp[:, V:] = 1e30
        lp[:, EOS] = -4000.0
        for r in range(n * nb):
            i = r // nb
            top = -np.sort(np.partition(-lp[r, :V], nb + 2)[:nb + 3])          # the row's largest values, descending
            if i == 0 and t >= 1:
                lp[r, EOS] = 0.0
            elif i == 1 and (t == 0 or rng.rand() < 0.5):
                lp[r, EOS] = top[rng.randint(0, min(nb + 2, V - 1))]
            elif i == 2 and t < 2:
                lp[r, EOS] = -np.inf
            elif i == 2 and rng.rand() < 0.15:
                lp[r, EOS] = top[rng.randint(0, nb)]
        lps.append(lp)
    return lps


class PoolBeamRef:
    """State, history and pools of a search with n_inst instances of n_bm beams over Tmax positions.
      scores [n, nb] f32, tokens [n, nb] i64, src [n * nb] i64, done [n] u8, length [n] i64, hist_* [Tmax, n, nb] (marker -7),
      pool[i]: a list of (key f32, raw f32, end_t, beam, finished) in SLOT order (arrival order, replacements in place)."""

    def __init__(self, n_inst, n_bm, V, Tmax, alpha, early_stopping=False, eos=-1, max_len=None, scores=None, tokens=None, done=None,
                 length=None):
        self.n, self.nb, self.V, self.Tmax, self.eos = n_inst, n_bm, V, Tmax, eos
        self.w, self.early = weights(alpha, Tmax), bool(early_stopping)
        self.max_len = Tmax if max_len is None else max_len
        self.scores = np.zeros((n_inst, n_bm), dtype=F32) if scores is None else np.array(scores, dtype=F32).reshape(n_inst, n_bm)
        self.tokens = np.zeros((n_inst, n_bm), dtype=np.int64) if tokens is None else np.array(tokens, dtype=np.int64).reshape(n_inst, n_bm)
        self.done = np.zeros(n_inst, dtype=np.uint8) if done is None else np.array(done, dtype=np.uint8).reshape(n_inst)
        self.length = np.zeros(n_inst, dtype=np.int64) if length is None else np.array(length, dtype=np.int64).reshape(n_inst)
        self.src = np.arange(n_inst * n_bm, dtype=np.int64)
        self.hist_par = np.full((Tmax, n_inst, n_bm), -7, dtype=np.int64)
        self.hist_tok = np.full((Tmax, n_inst, n_bm), -7, dtype=np.int64)
        self.hist_sc = np.full((Tmax, n_inst, n_bm), -7.0, dtype=F32)
        self.pool = [[] for _ in range(n_inst)]
        self.events, self.where = set(), ""

    def offer(self, pool, entry):
        """Append while there is room; else replace the last entry in pool order if the new one stands in front of it."""
        if len(pool) < self.nb:
            pool.append(entry)
            return
        last = pool_sorted(pool)[-1]
        if before(entry, last):
            pool[pool.index(last)] = entry
            self.events.add(self.where + "replacement")
        else:
            self.events.add(self.where + "drop")

    def step(self, lp, t, first=None):
        """lp: [n_inst * n_bm, >= V] fp32; only columns < V are candidates."""
        n, nb, V, eos = self.n, self.nb, self.V, self.eos
        first = (t == 0) if first is None else first
        lp = np.asarray(lp, dtype=F32)
        for i in range(n):
            if self.done[i]:                                  # frozen: state and pool untouched, identity parents
                self.src[i * nb:(i + 1) * nb] = i * nb + np.arange(nb)
                self.hist_par[t, i] = np.arange(nb)
                self.hist_tok[t, i] = self.tokens[i]
                self.hist_sc[t, i] = self.scores[i]
                continue
            rows = lp[i * nb:i * nb + (1 if first else nb), :V]
            value = rows.copy() if first else (rows + self.scores[i][:, None]).astype(F32)      # one fp32 addition
            flat = value.reshape(-1)
            order = np.argsort(-flat, kind="stable")          # larger value first, then lower flat index
            order = order[flat[order] != NEG_INF]            # a value of -inf is not a candidate
            if 0 <= eos < V and len([f for f in range(eos, flat.size, V) if flat[f] == NEG_INF]):
                self.events.add("inf_end_not_pooled")
            live, rank_of_end = [], []
            for rank, f in enumerate(order):
                f = int(f)
                if f % V == eos:
                    rank_of_end.append((rank, f))
                elif len(live) < nb:
                    live.append(f)
                if rank > nb and len(live) == nb:             # nothing further down the list is looked at
                    break
            ends_on_top = 0
            for rank, f in rank_of_end:                       # in candidate order
                if rank == nb:
                    self.events.add("end_at_rank_nb_not_taken")
                if rank >= nb:
                    continue
                if rank == nb - 1:
                    self.events.add("end_at_rank_nb_minus_1_taken")
                if t == 0:
                    self.events.add("end_at_t0")
                raw = flat[f]
                self.offer(self.pool[i], (F32(raw * self.w[t + 1]), F32(raw), t, f // V, 1))
                ends_on_top += 1
            if not first and 0 <= eos < V and all(int(np.argmax(value[b])) == eos for b in range(nb)):
                self.events.add("all_rows_end_best")
            assert len(live) == nb, "the caller's condition: n_bm finite non-end columns per live row"
            live = np.array(live, dtype=np.int64)
            self.scores[i] = flat[live]
            self.tokens[i] = live % V
            self.src[i * nb:(i + 1) * nb] = i * nb + live // V
            self.hist_par[t, i] = live // V
            self.hist_tok[t, i] = live % V
            self.hist_sc[t, i] = flat[live]
            self.length[i] += 1
            pool = self.pool[i]
            if len(pool) == nb:
                last = pool_sorted(pool)[-1]
                if self.early:
                    self.done[i] = 1
                    self.events.add("done_by_early_stopping")
                elif F32(self.scores[i, 0] * self.w[self.max_len]) <= last[0]:
                    self.done[i] = 1
                    self.events.add("done_by_bound")
            srt = pool_sorted(pool)
            for a, b in zip(srt, srt[1:]):
                if a[0] == b[0]:
                    self.events.add("equal_key_by_end_t" if a[2] != b[2] else "equal_key_by_beam")

    def pool_arrays(self):
        """The pool as the device holds it: key, raw [n, nb] f32, end_t, beam, finished [n, nb] i64 in slot order, count [n]; slots at
        or past the count are None-masked by the caller (mask [n, nb] bool)."""
        n, nb = self.n, self.nb
        key, raw = np.zeros((n, nb), dtype=F32), np.zeros((n, nb), dtype=F32)
        end_t, beam, fin = (np.zeros((n, nb), dtype=np.int64) for _ in range(3))
        mask = np.zeros((n, nb), dtype=bool)
        for i, pool in enumerate(self.pool):
            for s, e in enumerate(pool):
                key[i, s], raw[i, s], end_t[i, s], beam[i, s], fin[i, s], mask[i, s] = e[0], e[1], e[2], e[3], e[4], True
        return dict(key=key, raw=raw, end_t=end_t, beam=beam, finished=fin, count=mask.sum(1), mask=mask)

    def finish(self, n_best):
        """The live beams of every instance that is not done enter its pool (a copy: the pool itself is left as it is); then the first
        n_best entries in pool order: tokens [n, n_best, Tmax] (-1 padded; a finished entry's walk-back is followed by the end token),
        raw, key [n, n_best] f32, lengths, finished [n, n_best] i64."""
        n, nb, T = self.n, self.nb, self.Tmax
        tok = np.full((n, n_best, T), -1, dtype=np.int64)
        raw, key = np.full((n, n_best), NEG_INF, dtype=F32), np.full((n, n_best), NEG_INF, dtype=F32)
        lens, fin = np.zeros((n, n_best), dtype=np.int64), np.zeros((n, n_best), dtype=np.int64)
        self.where = "finish_"
        for i in range(n):
            pool = list(self.pool[i])
            if not self.done[i]:
                L = int(self.length[i])
                if L == T:
                    self.events.add("ran_to_Tmax_live_beams_pooled")
                for b in range(nb):
                    self.offer(pool, (F32(self.scores[i, b] * self.w[L]), F32(self.scores[i, b]), L, b, 0))
            for k, e in enumerate(pool_sorted(pool)[:n_best]):
                b = e[3]
                for j in range(e[2] - 1, -1, -1):
                    b = min(max(b, 0), nb - 1)
                    tok[i, k, j] = self.hist_tok[j, i, b]
                    b = int(self.hist_par[j, i, b])
                if e[4]:
                    tok[i, k, e[2]] = self.eos
                key[i, k], raw[i, k], lens[i, k], fin[i, k] = e[0], e[1], e[2] + (1 if e[4] else 0), e[4]
        self.where = ""
        return tok, raw, key, lens, fin


_CASES = {}


def run_case(nb, V, ld, offset, alpha, early):
    """(lps, the reference after all TMAX positions and the finish, the per-position snapshots, the finish's five outputs at
    n_best = n_bm) of one case of the kernel test; computed once."""
    key = (nb, V, ld, offset, alpha, early)
    if key not in _CASES:
        lps = make_lps(case_seed(nb, V, offset, alpha, early), nb, V, ld)
        ref = PoolBeamRef(N_INST, nb, V, TMAX, alpha, early, eos=EOS)
        snaps = []
        for t in range(TMAX):
            ref.step(lps[t], t)
            snaps.append(dict(scores=ref.scores.copy(), tokens=ref.tokens.copy(), src=ref.src.copy(), done=ref.done.copy(),
                              length=ref.length.copy(), hist_par=ref.hist_par[t].copy(), hist_tok=ref.hist_tok[t].copy(),
                              hist_sc=ref.hist_sc[t].copy(), pool=ref.pool_arrays()))
        _CASES[key] = (lps, ref, snaps, ref.finish(nb))
    return _CASES[key]
