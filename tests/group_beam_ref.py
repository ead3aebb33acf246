"""numpy restatement of the group beam step's contract (include/univl_hip.h: univl_beam_group_step), shared by
tests/test_group_beam_cpu.py (identities of the reference itself) and tests/test_group_beam_gpu.py (the kernel and the session bit for
bit).  Written from the header's words in np.float32 arithmetic.  Every group ranks ALL V columns of its rows by brute force -- never
through per-row candidate lists -- so that the kernel's argument that a row's top-n_bm list is enough is tested, not assumed.  It
shares no code with the package."""
import numpy as np

F32 = np.float32


def plain_topk(cand, k):
    """The k best of a flat fp32 vector, descending, equal values by LOWER index first: (values, indices)."""
    cand = np.asarray(cand, dtype=F32)
    order = np.argsort(-cand, kind="stable")[:k]
    return cand[order], order


class GroupBeamRef:
    """State and history of a search with n_inst instances, n_bm beams in G groups of k' = n_bm // G, over Tmax positions.
      scores [n_inst, n_bm] f32, tokens [n_inst, n_bm] i64, src [n_inst * n_bm] i64 (global rows), done / length [n_inst * G],
      hist_par (LOCAL to the group) / hist_tok [Tmax, n_inst, n_bm] i64, hist_sc f32.
    step(lp, t, first=None) applies one position; lam may be changed between steps."""

    def __init__(self, n_inst, n_bm, G, V, Tmax, lam, eos=-1, scores=None, tokens=None, done=None, length=None):
        assert n_bm % G == 0
        self.n, self.nb, self.G, self.kp, self.V, self.Tmax, self.lam, self.eos = n_inst, n_bm, G, n_bm // G, V, Tmax, F32(lam), eos
        P = n_inst * G
        self.scores = np.zeros((n_inst, n_bm), dtype=F32) if scores is None else np.array(scores, dtype=F32).reshape(n_inst, n_bm)
        self.tokens = np.zeros((n_inst, n_bm), dtype=np.int64) if tokens is None else np.array(tokens, dtype=np.int64).reshape(n_inst, n_bm)
        self.done = np.zeros(P, dtype=np.uint8) if done is None else np.array(done, dtype=np.uint8).reshape(P)
        self.length = np.zeros(P, dtype=np.int64) if length is None else np.array(length, dtype=np.int64).reshape(P)
        self.src = np.arange(n_inst * n_bm, dtype=np.int64)
        self.hist_par = np.full((Tmax, n_inst, n_bm), -7, dtype=np.int64)
        self.hist_tok = np.full((Tmax, n_inst, n_bm), -7, dtype=np.int64)
        self.hist_sc = np.full((Tmax, n_inst, n_bm), -7.0, dtype=F32)

    def step(self, lp, t, first=None):
        """lp: [n_inst * n_bm, >= V] fp32; only columns < V are candidates."""
        n, nb, G, kp, V = self.n, self.nb, self.G, self.kp, self.V
        first = (t == 0) if first is None else first
        lp = np.asarray(lp, dtype=F32)
        for i in range(n):
            count = np.zeros(V, dtype=np.int64)                   # c(v): beams of earlier LIVE groups that chose v at this position
            for g in range(G):
                b0, p = g * kp, i * G + g
                sl = slice(b0, b0 + kp)
                if self.done[p]:                                  # frozen: state untouched, identity parents, nothing added to c(v)
                    self.src[i * nb + b0:i * nb + b0 + kp] = i * nb + b0 + np.arange(kp)
                    self.hist_par[t, i, sl] = np.arange(kp)
                    self.hist_tok[t, i, sl] = self.tokens[i, sl]
                    self.hist_sc[t, i, sl] = self.scores[i, sl]
                    continue
                rows = lp[i * nb + b0:i * nb + b0 + (1 if first else kp), :V]
                value = rows.copy() if first else (rows + self.scores[i, sl][:, None]).astype(F32)      # one fp32 addition
                pen = (self.lam * count.astype(F32)).astype(F32)                                        # the product, rounded once
                ranked = (value - pen[None, :]).astype(F32)                                             # the difference, rounded separately
                _, pick = plain_topk(ranked.reshape(-1), kp)      # local flat index (b - b0) * V + v: the same order as b * V + v
                val = value.reshape(-1)[pick]
                order = np.lexsort((pick, -val))                  # re-sorted by the unpenalised value, ties by lower flat index
                pick, val = pick[order], val[order]
                parent, token = pick // V, pick % V
                self.scores[i, sl] = val
                self.tokens[i, sl] = token
                self.src[i * nb + b0:i * nb + b0 + kp] = i * nb + b0 + parent
                self.hist_par[t, i, sl] = parent
                self.hist_tok[t, i, sl] = token
                self.hist_sc[t, i, sl] = val
                self.length[p] += 1
                if token[0] == self.eos:
                    self.done[p] = 1
                np.add.at(count, token, 1)

    def hypotheses(self, n_best):
        """The walk-back per group: tokens [n_inst, G * n_best, Tmax] (-1 padded), scores [n_inst, G * n_best], lengths [n_inst, G]."""
        n, G, kp, T = self.n, self.G, self.kp, self.Tmax
        out = np.full((n, G * n_best, T), -1, dtype=np.int64)
        sc = np.zeros((n, G * n_best), dtype=F32)
        for i in range(n):
            for g in range(G):
                for k in range(n_best):
                    b = k
                    for j in range(int(self.length[i * G + g]) - 1, -1, -1):
                        out[i, g * n_best + k, j] = self.hist_tok[j, i, g * kp + b]
                        b = int(self.hist_par[j, i, g * kp + b])
                    sc[i, g * n_best + k] = self.scores[i, g * kp + k]
        return out, sc, self.length.reshape(n, G).copy()
