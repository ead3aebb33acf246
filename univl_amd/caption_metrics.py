"""Caption metrics without NLGEval: BLEU, ROUGE_L and CIDEr from device-side n-gram overlap statistics.

main_task_caption.py:612-618 ends an evaluation epoch with nlgEvalObj.compute_metrics(ref_list, hyp_list) and returns Bleu_4, which
the training loop uses to pick the best checkpoint (:673-677).  NLGEval is a Java-backed package; CaptionMetrics has its
compute_metrics signature and needs nothing but this library.  One launch of univl_caption_overlap (csrc/metric.hip) produces, per item,
the clipped n-gram counts, the two lengths, the longest common subsequences, ROUGE_L and CIDEr; the corpus arithmetic of BLEU and the
means are a few float64 operations on the host.

The formulas are the contract (include/univl_hip.h: UnivlCaptionOverlap).  They restate the bleu_scorer.py,
rouge.py and cider_scorer.py that NLGEval vendors, but NOTHING HERE HAS BEEN COMPARED WITH NLGEval ITSELF: the package cannot be
installed where this project is built and tested.  Someone who has it can compare on the hyp.txt / ref.txt that eval.eval_caption
writes.  METEOR needs Java and WordNet and is not computed: the result carries "METEOR": nan, so that the reference's log line formats.

consensus() is the second consumer of the same kernel: it picks, per video, the sampled caption that agrees most with the other samples
(minimum-Bayes-risk selection) from the rows CaptionSampler.sample() left on the device, without a host read.
"""
import warnings

import numpy as np
import torch

from . import ops
from ._lib import OVERLAP_SYM_MAX, OVERLAP_TMAX

KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "METEOR", "ROUGE_L", "CIDEr")


def _pack(rows):
    """Lists of integer rows -> (sym [rows, T] int32 zero padded, len [rows] int32), T = the longest row (at least 1)."""
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    T = max(1, int(lens.max()) if len(rows) else 1)
    if T > OVERLAP_TMAX:
        raise ValueError("caption metrics: a row of %d symbols; the kernel carries at most %d" % (T, OVERLAP_TMAX))
    sym = np.zeros((len(rows), T), dtype=np.int32)
    for i, r in enumerate(rows):
        if len(r):
            sym[i, :len(r)] = r
    if sym.size and (int(sym.min()) < 0 or int(sym.max()) > OVERLAP_SYM_MAX):
        raise ValueError("caption metrics: symbols must lie in [0, %d]" % OVERLAP_SYM_MAX)
    return sym, lens


def document_frequency(sym, lens, ref_begin, ref_rows):
    """The CIDEr tables on the host: for n = 1 .. 4 the number of ITEMS whose reference set holds each n-gram.  Returns (keys uint64
    ascending, counts int32, df_begin [5]): the four per-n tables one after the other (keys of a larger n are larger numbers)."""
    rows, T = sym.shape
    s = np.zeros((rows, T + 3), dtype=np.uint64)
    s[:, :T] = np.where(np.arange(T)[None, :] < lens[:, None], sym.astype(np.int64) + 1, 0).astype(np.uint64)
    word = s[:, :T] | (s[:, 1:T + 1] << np.uint64(16)) | (s[:, 2:T + 2] << np.uint64(32)) | (s[:, 3:T + 3] << np.uint64(48))
    item_of_ref = np.repeat(np.arange(len(ref_begin) - 1), np.diff(ref_begin))
    keys, cnts, begin = [], [], [0]
    for n in range(1, 5):
        mask = np.uint64(0xFFFFFFFFFFFFFFFF) if n == 4 else np.uint64((1 << (16 * n)) - 1)
        valid = (np.arange(T)[None, :] + n) <= lens[ref_rows][:, None]                     # [n_refs, T]
        k = (word[ref_rows] & mask)[valid]
        it = np.broadcast_to(item_of_ref[:, None], valid.shape)[valid]
        if k.size:
            order = np.lexsort((k, it))
            k, it = k[order], it[order]
            distinct = np.ones(k.size, dtype=bool)
            distinct[1:] = (k[1:] != k[:-1]) | (it[1:] != it[:-1])                          # one entry per (item, n-gram)
            uk, uc = np.unique(k[distinct], return_counts=True)
        else:
            uk, uc = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
        keys.append(uk.astype(np.uint64))
        cnts.append(uc.astype(np.int32))
        begin.append(begin[-1] + int(uk.size))
    return np.concatenate(keys), np.concatenate(cnts), begin


class DocumentFrequency:
    """CIDEr's document-frequency tables on the device, built there by ops.ngram_df (include/univl_hip.h: univl_ngram_df).  Owns keys
    (int64 storage of the ascending uint64 keys), cnt (int32), begin (five HOST ints: the n-grams are entries begin[n-1] .. begin[n))
    and n_docs; `.tables` is what ops.caption_overlap(tables=...) takes.  Building reads the five begin words and the status word on
    the host, once; using the tables (rl.caption_rewards(metric="cider", df=...)) reads nothing."""

    def __init__(self, keys, cnt, begin, n_docs):
        self.keys, self.cnt, self.begin, self.n_docs = keys, cnt, [int(b) for b in begin], int(n_docs)

    @property
    def tables(self):
        return (self.keys, self.cnt, self.begin, self.n_docs)

    @property
    def device(self):
        return self.keys.device

    @classmethod
    def _build(cls, sym, lens, ref_begin, ref_rows, n_refs, n_docs):
        """One ops.ngram_df launch, then the ONE host read: df_begin and the status word together."""
        keys, cnt, begin_dev, status = ops.ngram_df(sym, lens, ref_begin, ref_rows, n_refs)
        head = torch.cat([begin_dev, status]).cpu().tolist()
        if head[5]:
            raise RuntimeError("document frequency: the kernel flagged its input (status %d)" % head[5])
        n = head[4]
        return cls(keys[:n].clone(), cnt[:n].clone(), head[:5], n_docs)           # narrowed: the sufficient bound is not kept alive

    @classmethod
    def from_ids(cls, ref_ids, ref_len, device="cuda"):
        """ref_ids [n, n_ref, T] / ref_len [n, n_ref] integer tensors, on the device or the host: one document per video, the layout
        rl.caption_rewards takes its references in.  Positions past a length are not read."""
        if ref_ids.dim() != 3 or min(ref_ids.shape) < 1 or tuple(ref_len.shape) != tuple(ref_ids.shape[:2]):
            raise ValueError("document frequency: ref_ids of shape %s / ref_len of shape %s, expected [n, n_ref, T] / [n, n_ref], each "
                             "dimension >= 1" % (tuple(ref_ids.shape), tuple(ref_len.shape)))
        if ref_ids.is_floating_point() or ref_len.is_floating_point():
            raise ValueError("document frequency: ref_ids / ref_len must be integer tensors")
        n, n_ref, T = (int(v) for v in ref_ids.shape)
        if T > OVERLAP_TMAX:
            raise ValueError("document frequency: rows of %d positions; the kernel carries at most %d" % (T, OVERLAP_TMAX))
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("DocumentFrequency needs a HIP device (got %s, available: %s); there is no CPU fallback"
                               % (dev, torch.cuda.is_available()))
        with torch.cuda.device(dev):
            sym = ref_ids.to(dev).reshape(n * n_ref, T).to(torch.int32).contiguous()
            lens = ref_len.to(dev).reshape(n * n_ref).to(torch.int32).contiguous()
            ref_begin = torch.arange(n + 1, dtype=torch.int32, device=dev) * n_ref
            ref_rows = torch.arange(n * n_ref, dtype=torch.int32, device=dev)
            return cls._build(sym, lens, ref_begin, ref_rows, n * n_ref, n)

    @classmethod
    def from_lists(cls, ref_lists, device="cuda"):
        """ref_lists[i]: the integer rows of document i (Python lists; a document may be empty).  Packed as CaptionMetrics packs."""
        if len(ref_lists) == 0:
            raise ValueError("document frequency: at least one document is needed")
        rows = [list(r) for refs in ref_lists for r in refs]
        if not rows:
            raise ValueError("document frequency: at least one row is needed")
        sym, lens = _pack(rows)
        ref_begin = np.zeros(len(ref_lists) + 1, dtype=np.int32)
        ref_begin[1:] = np.cumsum([len(r) for r in ref_lists])
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("DocumentFrequency needs a HIP device (got %s, available: %s); there is no CPU fallback"
                               % (dev, torch.cuda.is_available()))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        with torch.cuda.device(dev):
            return cls._build(up(sym), up(lens), up(ref_begin), up(np.arange(len(rows), dtype=np.int32)), len(rows), len(ref_lists))

    def to_host(self):
        """(keys uint64 ascending, counts int32, begin [5]): document_frequency's form."""
        return self.keys.cpu().numpy().view(np.uint64), self.cnt.cpu().numpy(), list(self.begin)


def corpus_scores(guess, correct, hyp_len, ref_len, rouge_l, cider):
    """The corpus arithmetic, float64 on the host, from the per-item results (host arrays)."""
    out = {}
    bleu = 1.0
    ratio = (float(hyp_len.sum()) + 1e-15) / (float(ref_len.sum()) + 1e-9)
    for k in range(4):
        bleu *= (float(correct[:, k].sum()) + 1e-15) / (float(guess[:, k].sum()) + 1e-9)
        b = bleu ** (1.0 / (k + 1))
        if ratio < 1:
            b *= float(np.exp(1 - 1 / ratio))
        out["Bleu_%d" % (k + 1)] = b
    out["METEOR"] = float("nan")
    out["ROUGE_L"] = float(np.mean(rouge_l))
    out["CIDEr"] = float(np.mean(cider))
    return out


class CaptionMetrics:
    """NLGEval's compute_metrics on this library.  The constructor accepts and ignores NLGEval's keywords (no_overlap, no_skipthoughts,
    no_glove, metrics_to_omit, ...).  `last` holds the per-item host arrays of the most recent call.
    truncate: a row of more than 128 symbols is a ValueError by default; with truncate=True it is cut to its first 128 and a
    UserWarning says how many rows were cut (the launcher shim's stub asks for this: its call comes at the END of an evaluation epoch,
    after the whole test set was decoded, and one over-long caption must not cost the epoch).
    df: "host" (the default) builds CIDEr's document-frequency tables with document_frequency (numpy), "device" with ops.ngram_df
    (DocumentFrequency); the tables, and so the results, are the same.
    Arguments are validated on the host BEFORE a device is asked for, so malformed input is a ValueError with or without a GPU."""

    def __init__(self, device="cuda", truncate=False, df="host", **nlgeval_keywords):
        if df not in ("host", "device"):
            raise ValueError("CaptionMetrics: df=%r, expected 'host' (document_frequency, numpy) or 'device' (ops.ngram_df)" % (df,))
        self.device = torch.device(device)
        self.truncate = bool(truncate)
        self.df = df
        self.last = None

    def compute_ids(self, hyp_ids, ref_ids):
        """hyp_ids[i]: the integer row of item i's hypothesis; ref_ids[i]: the list of item i's reference rows (at least one).
        Symbols in [0, 65534], rows of at most 128.  Returns the seven-key dictionary."""
        items = len(hyp_ids)
        if items == 0 or len(ref_ids) != items:
            raise ValueError("caption metrics: %d hypotheses for %d reference lists (at least one item)" % (items, len(ref_ids)))
        if any(len(r) == 0 for r in ref_ids):
            raise ValueError("caption metrics: every item needs at least one reference")
        rows = [list(h) for h in hyp_ids] + [list(r) for refs in ref_ids for r in refs]
        if self.truncate:
            cut = sum(1 for r in rows if len(r) > OVERLAP_TMAX)
            if cut:
                warnings.warn("caption metrics: %d of %d rows hold more than %d symbols and were cut to their first %d"
                              % (cut, len(rows), OVERLAP_TMAX, OVERLAP_TMAX))
                rows = [r[:OVERLAP_TMAX] for r in rows]
        sym, lens = _pack(rows)
        ref_begin = np.zeros(items + 1, dtype=np.int32)
        ref_begin[1:] = np.cumsum([len(r) for r in ref_ids])
        n_refs = int(ref_begin[-1])
        ref_rows = np.arange(items, items + n_refs, dtype=np.int32)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("CaptionMetrics needs a HIP device (got %s, available: %s); there is no CPU fallback"
                               % (self.device, torch.cuda.is_available()))
        dev = self.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if self.df == "host":
            keys, cnts, begin = document_frequency(sym, lens, ref_begin, ref_rows)
            tables = (up(keys.view(np.int64)), up(cnts), begin, items)
        with torch.cuda.device(dev):
            sym_d, lens_d, ref_begin_d, ref_rows_d = up(sym), up(lens), up(ref_begin), up(ref_rows)
            if self.df == "device":
                tables = DocumentFrequency._build(sym_d, lens_d, ref_begin_d, ref_rows_d, n_refs, items).tables
            o = ops.caption_overlap(sym_d, lens_d, up(np.arange(items, dtype=np.int32)), ref_begin_d, ref_rows_d, n_refs, tables=tables)
        host = {k: v.cpu().numpy() for k, v in o.items() if v is not None}
        if int(host["status"][0]):
            raise RuntimeError("caption metrics: the kernel flagged its input (status %d)" % int(host["status"][0]))
        self.last = host
        return corpus_scores(host["guess"], host["correct"], host["hyp_len"], host["ref_len"], host["rouge_l"], host["cider"])

    def compute_metrics(self, ref_list, hyp_list):
        """NLGEval's call: ref_list[r][i] is reference r of item i -- one list for single-reference data, the zip(*...) of
        main_task_caption.py:599-609 for MSRVTT; hyp_list[i] is item i's hypothesis.  Strings are split on whitespace and words get ids
        in first-seen order."""
        ids = {}

        def row(text):
            out = []
            for w in text.split():
                k = ids.get(w)
                if k is None:
                    k = ids[w] = len(ids)
                    if k >= OVERLAP_SYM_MAX:
                        raise ValueError("caption metrics: more than %d distinct words" % OVERLAP_SYM_MAX)
                out.append(k)
            return out
        if any(len(refs) != len(hyp_list) for refs in ref_list) or not ref_list:
            raise ValueError("caption metrics: ref_list[r] must hold one reference per hypothesis (%d); got %s"
                             % (len(hyp_list), [len(refs) for refs in ref_list]))
        hyp_ids = [row(h) for h in hyp_list]
        ref_ids = [[row(refs[i]) for refs in ref_list] for i in range(len(hyp_list))]
        return self.compute_ids(hyp_ids, ref_ids)


_LAYOUTS = {}


def _consensus_layout(n, ns, dev):
    """Item tables of "every sample against the other samples of its video", built with device arithmetic once per shape."""
    key = (n, ns, str(dev))
    if key not in _LAYOUTS:
        rows = n * ns
        item = torch.arange(rows, dtype=torch.int32, device=dev)
        other = torch.arange(ns - 1, dtype=torch.int32, device=dev)[None, :]
        s = (item % ns)[:, None]
        refs = (item - item % ns)[:, None] + other + (other >= s).to(torch.int32)          # the ns - 1 rows of the video that are not s
        _LAYOUTS[key] = (item, torch.arange(rows + 1, dtype=torch.int32, device=dev) * (ns - 1), refs.reshape(-1).contiguous())
    return _LAYOUTS[key]


def consensus(sample_result, eos, pad, metric="rouge_l", eos_dev=None):
    """Minimum-Bayes-risk selection among sampled captions.  On the rows of SampleResult.captions(eos, pad) -- PIECE ids after the cut,
    not words: "##" continuation pieces count as symbols of their own -- every sample is scored against the other n_samp - 1 samples of
    its video (metric "rouge_l": the kernel's ROUGE_L with them as references; "bleu": the sentence BLEU-4 of its own counts), and
    univl_consensus_pick takes the best, equal scores to the lower index.  Returns device tensors (index [n] int32, score [n] fp64);
    nothing is read on the host (so the launch's status word is not looked at: piece ids above 65534 would be clamped)."""
    if metric not in ("rouge_l", "bleu"):
        raise ValueError("consensus: metric=%r, expected 'rouge_l' or 'bleu'" % (metric,))
    cap, cap_len = sample_result.captions(eos, pad, eos_dev=eos_dev)
    n, ns, Tmax = cap.shape
    if ns < 2:
        raise ValueError("consensus: %d sample per video; at least 2 are needed" % ns)
    if Tmax > OVERLAP_TMAX:
        raise ValueError("consensus: rows of %d positions; the kernel carries at most %d" % (Tmax, OVERLAP_TMAX))
    hyp_row, ref_begin, ref_rows = _consensus_layout(n, ns, cap.device)
    o = ops.caption_overlap(cap.view(n * ns, Tmax), cap_len.reshape(n * ns), hyp_row, ref_begin, ref_rows, n * ns * (ns - 1),
                            bleu=(metric == "bleu"))
    return ops.consensus_pick((o["bleu"] if metric == "bleu" else o["rouge_l"]).view(n, ns))
