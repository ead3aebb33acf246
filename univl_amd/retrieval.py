"""Retrieval search: build a gallery once, search it many times -- the retrieval counterpart of decode.CaptionBeamSearch.

VideoIndex holds one pooled (and, unless use_mil, L2-normalised) 768-wide fp32 vector per video in ONE device buffer that doubles
when full; a query is pooled the same way get_similarity_logits pools it (modeling.py:377-391) and searched with univl_sim_topk
(include/univl_hip.h): the k best gallery rows per query, sorted by descending score, equal scores by lower row id first, without the
[queries, gallery] matrix.  The opposite direction is the same code: fill an index with text vectors through add_vectors and query it
with video vectors through search_vectors.

Stage-two / train_sim_after_cross models score a pair through the cross encoder; search(..., rerank=True) runs only the k joint-head
candidates of every query through it (queries x k pairs instead of queries x gallery) and re-sorts each row by the cross score.

QueryBank is the search-time remedy against hubness (query-bank normalisation, the dynamic inverted softmax): a bank of other texts
-- training captions, say -- states how strongly every video is already claimed, and search(..., bank=) ranks by the score minus that
column term (include/univl_hip.h: univl_sim_colstat, univl_sim_topk_norm).  No retraining, and no [bank, gallery] matrix.

Moment search says WHERE in a video a text matches: VideoIndex(keep_frames=True).localize() scores every window of frames of a
candidate video the way get_similarity_logits scores the whole video (include/univl_hip.h: univl_window_norms,
univl_moment_localize) and returns the best one -- or, with n_best=, the n best after temporal non-maximum suppression
(univl_moment_nbest); search_moments() does that for the best videos of a search and ranks the moments.

Step alignment says where every step of an ORDERED list of texts happens: align_steps() places all of them at once, in order and
without overlap, by the same window score (univl_step_align) -- action step localisation.

Segmentation asks from the video's side: segment() gives every frame of a video one of a SET of label texts or the background, by the
one-frame window score and a penalty per change of label (univl_frame_segment) -- action segmentation, in its zero-shot form.

Video alignment needs no text: align_videos() lays the frames of one gallery video over those of another, monotonically
(univl_video_align: DTW, or with local=True the best common segment), and transfer_labels() carries an exemplar's frame labels across."""
import collections
import ctypes
import math
import numbers

import torch

from . import _lib, ops

H = 768
_NMS = (1, 2)              # the default suppression threshold of n-best localisation: temporal IoU above 1 / 2 (check_nbest knows it by identity)


class _DefaultTau(float):
    """align_videos' default tau, told from a 1.0 the caller wrote by identity: local=True accepts no default."""


_TAU_DTW = _DefaultTau(1.0)
VideoAlignment = collections.namedtuple("VideoAlignment", "score path_len path_a path_b match match_score")


class VideoIndex:
    def __init__(self, model, capacity=1024, keep_frames=False):
        """capacity: rows allocated at first (the buffer doubles when full); keep_frames: also keep every video's visual_output and
        mask, which rerank=True needs."""
        if capacity < 1:
            raise ValueError("VideoIndex: capacity must be at least 1")
        self.model, self.keep_frames = model, bool(keep_frames)
        self._cap, self._n = int(capacity), 0
        self._buf = self._frames = self._fmask = None
        self._wnorm, self._wnorm_rows = None, 0          # localize(): the window-norm table and how many rows of it are filled

    def __len__(self):
        return self._n

    @property
    def vectors(self):
        """[len(index), 768] fp32 view of the filled rows."""
        return self._reserve(0)[:self._n]

    @property
    def normalize(self):
        return not bool(self.model.task_config.use_mil)

    def _device(self):
        return self.model.flat.device

    def _reserve(self, extra, F=None):
        """Room for `extra` more rows; growth copies the filled rows on the device."""
        dev, cap, n = self._device(), self._cap, self._n
        while n + extra > cap:
            cap *= 2
        if self._buf is None or cap != self._cap:
            self._buf = _grown(self._buf, n, cap, H, device=dev)
        if self.keep_frames and F is not None:
            if self._frames is not None and self._frames.shape[1] != F:
                raise ValueError("VideoIndex: videos of %d frames in an index of %d-frame videos" % (F, self._frames.shape[1]))
            if self._frames is None or self._frames.shape[0] != cap:
                self._frames = _grown(self._frames, n, cap, F, H, device=dev)
                self._fmask = _grown(self._fmask, n, cap, F, device=dev, dtype=torch.int64, zero=True)
                if self._wnorm is not None:
                    self._wnorm = _grown(self._wnorm, self._wnorm_rows, cap, F, F, device=dev)
        self._cap = cap
        return self._buf

    def _ids(self, b):
        ids = torch.arange(self._n, self._n + b, device=self._device(), dtype=torch.int32)
        self._n += b
        return ids

    @torch.no_grad()
    def add(self, video, video_mask):
        """Encodes the videos (UniVL.get_visual_output: the text stack does not run), pools them as get_similarity_logits does and
        appends them.  Returns their row ids (int32 device tensor)."""
        F = video_mask.shape[-1]
        vo = self.model.get_visual_output(video, video_mask)
        b, dev = vo.shape[0], vo.device
        vm = video_mask.reshape(-1, F).to(dev, torch.int64).contiguous()
        buf = self._reserve(b, F)
        ops.pool_fwd(b, F, vo, vm, skip_first=False, normalize=self.normalize, out=buf[self._n:self._n + b])
        if self.keep_frames:
            self._frames[self._n:self._n + b].copy_(vo)
            self._fmask[self._n:self._n + b].copy_(vm)
        return self._ids(b)

    @torch.no_grad()
    def add_vectors(self, vectors):
        """Appends pooled vectors the caller already holds ([b, 768]; e.g. text vectors for video-to-text search)."""
        if self.keep_frames:
            raise ValueError("VideoIndex.add_vectors: an index that keeps frames is filled through add()")
        v = vectors.reshape(-1, H)
        self._reserve(v.shape[0])[self._n:self._n + v.shape[0]].copy_(v)
        return self._ids(v.shape[0])

    @torch.no_grad()
    def pool_text(self, input_ids, token_type_ids, attention_mask):
        """(pooled query vectors [Nq, 768], sequence_output, mask): the text through UniVL.get_sequence_output (the video stack does
        not run) and the masked mean without the first token."""
        W = input_ids.shape[-1]
        so = self.model.get_sequence_output(input_ids, token_type_ids, attention_mask)
        am = attention_mask.reshape(-1, W).to(so.device, torch.int64).contiguous()
        q = torch.empty(so.shape[0], H, device=so.device, dtype=torch.float32)
        ops.pool_fwd(so.shape[0], W, so, am, skip_first=True, normalize=self.normalize, out=q)
        return q, so, am

    @torch.no_grad()
    def search(self, input_ids, token_type_ids, attention_mask, k=10, targets=None, rerank=False, chunk_rows=5, bank=None):
        """The k best videos for every text.  Returns (scores [Nq, k] fp32, indices [Nq, k] int32) on the device, rows sorted by
        descending score, equal scores by lower row id first, -inf / -1 past the end of a gallery smaller than k.  With targets
        ([Nq] gallery rows) it also returns (gt, eq), the rank counts of every query's target (k = 0: only those).
        rerank=True (keep_frames=True, a model with a cross encoder, k <= len(index)): the k joint-head candidates are scored by
        the cross encoder, chunk_rows queries at a time; returns the cross scores and the re-ordered row ids.
        bank: a fitted QueryBank of this index; scores, order and rank counts are then those of the normalised score (QueryBank),
        and rerank=True takes its candidates from the normalised search.  A bank whose fit() is stale is a ValueError."""
        if bank is not None:
            bank.check_fitted(self)
        q, so, am = self.pool_text(input_ids, token_type_ids, attention_mask)
        if rerank:
            if targets is not None:
                raise ValueError("VideoIndex.search: rank counts are taken from the joint head; call without rerank for them")
            return self._rerank(q, so, am, int(k), int(chunk_rows), bank)
        return self.search_vectors(q, k, targets, bank)

    @torch.no_grad()
    def search_vectors(self, q, k, targets=None, bank=None):
        """search() for pooled query vectors the caller already holds ([Nq, 768] fp32 on the index's device)."""
        if self._n == 0:
            raise ValueError("VideoIndex: the index is empty")
        if bank is not None:
            bank.check_fitted(self)
        q = _query_rows(q)
        if targets is not None:
            targets = torch.as_tensor(targets).reshape(-1).to(device=q.device, dtype=torch.int32).contiguous()
        if bank is None:
            return ops.sim_topk(q, self.vectors, int(k), target=targets)
        # plain top-1 -> gate -> normalised scan; a static bank has no gates and is the last launch pair alone
        gate = ops.hub_gate(ops.sim_topk(q, self.vectors, 1)[1], bank.hub) if bank.dynamic else None
        return ops.sim_topk_norm(q, self.vectors, int(k), bank.c, row_gate=gate, target=targets)

    def _rerank(self, q, so, am, K, chunk_rows, bank=None):
        from .steps import EvalSession, PoolerSim
        model = self.model
        if model.cross is None:
            raise ValueError("VideoIndex.search(rerank=True): this model has no cross encoder")
        if not self.keep_frames or self._frames is None:
            raise ValueError("VideoIndex.search(rerank=True) needs an index built with keep_frames=True")
        if not 1 <= K <= min(self._n, _lib.TOPK_MAX):
            raise ValueError("VideoIndex.search(rerank=True): k=%d, need 1 <= k <= min(len(index), %d)" % (K, _lib.TOPK_MAX))
        _, idx = self.search_vectors(q, K, None, bank)
        Nq, W = so.shape[0], so.shape[1]
        F = self._frames.shape[1]
        cross = torch.empty(Nq, K, device=q.device, dtype=torch.float32)
        for lo in range(0, Nq, chunk_rows):
            n = min(chunk_rows, Nq - lo)
            ses = model._eval_session(("rerank", n, K, W, F), lambda: EvalSession(
                model, n, n * K, W, F, [i for i in range(n) for _ in range(K)], list(range(n * K)), PoolerSim, n, K, None))
            feats = ses.feats
            cand = idx[lo:lo + n].reshape(-1).contiguous()
            ops.gather_rows(self._frames, feats.vis_out, cand, n * K, F * H * 4, F * H * 4)
            feats.vmask.copy_(self._fmask.index_select(0, cand.long()))
            feats.seq_out.copy_(so[lo:lo + n].reshape(n * W, H))
            feats.amask.copy_(am[lo:lo + n])
            ses.plan.run()
            cross[lo:lo + n].copy_(ses.head.sim.view(n, K))
        sc, order = _rank_rows(cross, idx)                # k <= len(index): no empty slot among the candidates
        return sc, idx.gather(1, order)

    # ------------------------------------------------------------------------------------------ moment search
    def _window_norms(self):
        """[len(index), F, F] window norms (ops.window_norms), filled lazily: the table depends on the videos alone, so the rows added
        since the last call are computed and the others kept.  Allocated by the first localisation of a normalising model."""
        F = self._frames.shape[1]
        if self._wnorm is None:
            self._wnorm = _grown(None, 0, self._cap, F, F, device=self._device())
        lo, n = self._wnorm_rows, self._n
        if lo < n:
            ops.window_norms(self._frames[lo:n], self._fmask[lo:n], out=self._wnorm[lo:n])
            self._wnorm_rows = n
        return self._wnorm[:n]

    @torch.no_grad()
    def localize(self, input_ids, token_type_ids, attention_mask, rows, window, n_best=None, nms=_NMS):
        """The best-matching window of frames of gallery row rows[i, j] for text i.  rows: [Nq, K] int32 gallery rows, search()'s
        indices say; window = (lmin, lmax): the lengths searched, in frames.  Returns (start, length, score), each [Nq, K] on the
        device: the window whose masked mean -- normalised unless use_mil, as get_similarity_logits scores a whole video -- has the
        largest inner product with the pooled text; equal scores by lower start, then smaller length; (-1, 0, -inf) where no window of
        these lengths lies inside the valid frames, and for the -1 rows of a short search.  Needs keep_frames=True.
        n_best (an integer, 1 .. MOMENT_NBEST_MAX): SEVERAL windows per pair, each result [Nq, K, n_best] -- greedy temporal
        non-maximum suppression in one launch (include/univl_hip.h: univl_moment_nbest): the best window, then the best of those whose
        IoU in frames with every window taken so far is at most num / den, nms = (num, den) integers with 1 <= den <= 1024 and
        0 <= num <= den, decided in integers.  Slot 0 is the window of the call without n_best, scores never increase along a pair's
        slots, and the slots past the last survivor are (-1, 0, -inf).  nms=(1, 1) is the plain top n_best, (0, 1) disjoint windows."""
        check_nbest("VideoIndex.localize", n_best, nms)
        return self.localize_vectors(self.pool_text(input_ids, token_type_ids, attention_mask)[0], rows, window, n_best, nms)

    @torch.no_grad()
    def localize_vectors(self, q, rows, window, n_best=None, nms=_NMS):
        """localize() for pooled query vectors the caller already holds ([Nq, 768] fp32 on the index's device)."""
        check_nbest("VideoIndex.localize_vectors", n_best, nms)
        lmin, lmax = self._check_window("localize", window)
        q = _query_rows(q)
        rows = torch.as_tensor(rows).to(device=q.device, dtype=torch.int32).reshape(q.shape[0], -1).contiguous()
        wnorm = self._window_norms() if self.normalize else None
        frames, mask = self._frames[:self._n], self._fmask[:self._n]
        if n_best is None:
            return ops.moment_localize(q, frames, mask, rows, lmin, lmax, wnorm=wnorm, normalize=self.normalize)
        return ops.moment_nbest(q, frames, mask, rows, lmin, lmax, n_best, nms, wnorm=wnorm, normalize=self.normalize)

    def _check_window(self, who, window):
        """(lmin, lmax) of a localisation, or the ValueError every localiser raises: no frames kept, a bad window, videos too long."""
        if not self.keep_frames or self._frames is None:
            raise ValueError("VideoIndex.%s needs an index built with keep_frames=True, with videos in it" % who)
        F = self._frames.shape[1]
        lmin, lmax = (int(w) for w in window)
        if not 1 <= lmin <= lmax <= F:
            raise ValueError("VideoIndex.%s: window=(%d, %d), need 1 <= lmin <= lmax <= %d frames" % (who, lmin, lmax, F))
        if F > _lib.MOMENT_F_MAX:
            raise ValueError("VideoIndex.%s: videos of %d frames, at most %d" % (who, F, _lib.MOMENT_F_MAX))
        return lmin, lmax

    # ------------------------------------------------------------------------------------------ ordered step alignment
    @torch.no_grad()
    def align_steps(self, input_ids, token_type_ids, attention_mask, counts, rows, window=(1, 1)):
        """Where every step of an ORDERED list of texts happens in gallery row rows[i, c].  The text tensors are [Nl, K, W]: list i's
        steps are its first counts[i] texts, the others padding (encoded like any text, their vectors never read); K <= STEP_K_MAX.
        rows: [Nl, C] gallery rows; window = (lmin, lmax): the length of a step's window, in frames -- (1, 1) is one frame per step.
        Returns (start, length, score [Nl, C, K], total [Nl, C]) on the device: the windows, each scored as localize() scores it, in
        order and never overlapping, whose scores have the largest sum (include/univl_hip.h: univl_step_align); padding slots are
        (-1, 0, -inf); a video whose valid frames cannot hold all the steps is (-1, 0, -inf) in every slot with total -inf, and so is
        a -1 row or a count outside [1, K].  With one step per list the result is localize()'s.  Needs keep_frames=True."""
        Nl, K, _, _ = self._check_lists("align_steps", input_ids, window)
        flat = (t.reshape(Nl * K, -1) for t in (input_ids, token_type_ids, attention_mask))
        return self.align_vectors(self.pool_text(*flat)[0].view(Nl, K, H), counts, rows, window)

    @torch.no_grad()
    def align_vectors(self, q, counts, rows, window=(1, 1)):
        """align_steps() for pooled step vectors the caller already holds ([Nl, K, 768] fp32 on the index's device)."""
        Nl, K, lmin, lmax = self._check_lists("align_vectors", q, window)
        q = _query_rows(q).view(Nl, K, H)
        counts = torch.as_tensor(counts).to(device=q.device, dtype=torch.int32).reshape(Nl).contiguous()
        rows = torch.as_tensor(rows).to(device=q.device, dtype=torch.int32).reshape(Nl, -1).contiguous()
        wnorm = self._window_norms() if self.normalize else None
        return ops.step_align(q, counts, self._frames[:self._n], self._fmask[:self._n], rows, lmin, lmax, wnorm=wnorm, normalize=self.normalize)

    def _check_lists(self, who, lists, window, kmax=_lib.STEP_K_MAX):
        """(Nl, K, lmin, lmax) for a [Nl, K, .] tensor of step lists (or label sets of at most kmax), after every refusal that needs no
        device work."""
        lmin, lmax = self._check_window(who, window)
        if lists.dim() != 3:
            raise ValueError("VideoIndex.%s: step lists are [lists, steps, .] tensors, got %d dimensions" % (who, lists.dim()))
        if not 1 <= lists.shape[1] <= kmax:
            raise ValueError("VideoIndex.%s: lists of %d steps, need 1 .. %d" % (who, lists.shape[1], kmax))
        return lists.shape[0], lists.shape[1], lmin, lmax

    # ------------------------------------------------------------------------------------------ frame-wise segmentation
    @torch.no_grad()
    def segment(self, input_ids, token_type_ids, attention_mask, counts, rows, switch_penalty=0.0, background=None):
        """Which of a SET of texts, if any, every frame of gallery row rows[i, c] shows (action segmentation).  The text tensors are
        [Nl, K, W]: set i's labels are its first counts[i] texts, the others padding (encoded like any text, their vectors never read);
        K <= SEGMENT_K_MAX.  rows: [Nl, C] gallery rows.  A frame scores for a label what localize() scores that one-frame window;
        background: the score of "none of these" on every frame (None: no such label); switch_penalty >= 0 is paid at every change of
        label between neighbouring valid frames -- 0 is the arg-max of every frame by itself, a large one gives the video one label.
        Returns (label [Nl, C, F] int32: k, -1 background, -2 on a masked frame; score [Nl, C, F]: the chosen label's frame score; total
        [Nl, C]: the objective; nseg [Nl, C]: the runs of equal non-background labels) on the device (include/univl_hip.h:
        univl_frame_segment); a -1 row, a count outside [1, K] or a video without a valid frame is -2 / -inf throughout with total -inf
        and nseg 0.  Labels need no order and may repeat or be absent.  Needs keep_frames=True."""
        Nl, K = self._check_sets("segment", input_ids, switch_penalty, background)
        flat = (t.reshape(Nl * K, -1) for t in (input_ids, token_type_ids, attention_mask))
        return self.segment_vectors(self.pool_text(*flat)[0].view(Nl, K, H), counts, rows, switch_penalty, background)

    @torch.no_grad()
    def segment_vectors(self, q, counts, rows, switch_penalty=0.0, background=None):
        """segment() for pooled label vectors the caller already holds ([Nl, K, 768] fp32 on the index's device)."""
        Nl, K = self._check_sets("segment_vectors", q, switch_penalty, background)
        q = _query_rows(q).view(Nl, K, H)
        counts = torch.as_tensor(counts).to(device=q.device, dtype=torch.int32).reshape(Nl).contiguous()
        rows = torch.as_tensor(rows).to(device=q.device, dtype=torch.int32).reshape(Nl, -1).contiguous()
        wnorm = self._window_norms() if self.normalize else None
        return ops.frame_segment(q, counts, self._frames[:self._n], self._fmask[:self._n], rows, switch_penalty, background, wnorm=wnorm,
                                 normalize=self.normalize)

    def _check_sets(self, who, sets, switch_penalty, background):
        """(Nl, K) for a [Nl, K, .] tensor of label sets, after every refusal that needs no device work."""
        Nl, K, _, _ = self._check_lists(who, sets, (1, 1), _lib.SEGMENT_K_MAX)
        check_segment_args("VideoIndex.%s" % who, switch_penalty, background)
        return Nl, K

    # ------------------------------------------------------------------------------------------ video-to-video alignment
    @torch.no_grad()
    def align_videos(self, ref, rows, tau=_TAU_DTW, local=False):
        """A monotone alignment of the valid frames of gallery row ref[p] (the exemplar) with those of every gallery row rows[p, c].
        ref: [P] gallery rows; rows: [P, C] (or [P]: one candidate each).  The score of a pair of frames is their cosine minus tau --
        ALWAYS the cosine, also for a use_mil model: the model defines no video-video score.  local=False: the best path from the first
        valid frames of both to the last ones (tau = 1: classic DTW under the cosine distance).  local=True: the best-scoring common
        segment, free at both ends; tau is then what separates a match from a mismatch and MUST be given -- no default is invented
        for it.  Returns a VideoAlignment (score [P, C], path_len [P, C], path_a, path_b [P, C, 2 F]: the path's cells first to last as
        frame indices, -1 past path_len; match [P, C, F]: the exemplar frame every candidate frame is matched with, -1 not on the path,
        -2 masked; match_score [P, C, F]) on the device (include/univl_hip.h: univl_video_align); a -1 row or a video without a valid
        frame is (-inf, 0, -1, -1, -2, -inf) throughout.  Needs keep_frames=True."""
        check_valign_args("VideoIndex.align_videos", tau, local, tau is not _TAU_DTW)
        if not self.keep_frames or self._frames is None:
            raise ValueError("VideoIndex.align_videos needs an index built with keep_frames=True, with videos in it")
        ref = torch.as_tensor(ref)
        rows = torch.as_tensor(rows)
        if ref.dim() != 1 or ref.numel() == 0 or rows.dim() not in (1, 2) or rows.shape[0] != ref.shape[0] or rows.numel() == 0:
            raise ValueError("VideoIndex.align_videos: ref %s and rows %s (need [pairs] and [pairs, candidates], neither empty)"
                             % (tuple(ref.shape), tuple(rows.shape)))
        dev = self._frames.device
        ref = ref.to(device=dev, dtype=torch.int32).contiguous()
        rows = rows.to(device=dev, dtype=torch.int32).reshape(ref.shape[0], -1).contiguous()
        return VideoAlignment(*ops.video_align(self._frames[:self._n], self._fmask[:self._n], ref, rows, float(tau), bool(local)))

    @torch.no_grad()
    def transfer_labels(self, ref_labels, result):
        """Carries frame labels of the exemplars across an alignment: ref_labels [P, F] integers, the labels of the frames of ref[p];
        result: align_videos()'s.  Returns [P, C, F] int32: for every frame of every candidate the exemplar's label at match, where
        match >= 0; match's own -1 (not on the path) or -2 (masked) elsewhere.  A device gather, no host read."""
        match = result.match
        labels = torch.as_tensor(ref_labels).to(device=match.device, dtype=torch.int32)
        P, C, F = match.shape
        if labels.shape != (P, F):
            raise ValueError("VideoIndex.transfer_labels: ref_labels %s for an alignment of %d exemplars and %d frames"
                             % (tuple(labels.shape), P, F))
        got = torch.gather(labels.unsqueeze(1).expand(P, C, F), 2, match.clamp(min=0).to(torch.int64))
        return torch.where(match >= 0, got, match)

    @torch.no_grad()
    def search_moments(self, input_ids, token_type_ids, attention_mask, k=10, window=(1, 1), shortlist=None, bank=None, per_video=1, nms=_NMS):
        """The k best (video, window) moments for every text.  The `shortlist` (default k, at most TOPK_MAX) best videos by WHOLE-VIDEO
        score come from search_vectors -- through `bank` if one is given -- each is localised, and the shortlist is re-ordered by window
        score.  So the result is exhaustive over the index when shortlist >= len(index) and otherwise what it says: the best moments
        among the videos a whole-video search ranks first; a moment in a video that scores poorly as a whole is not found.
        Returns (score, idx, start, length), each [Nq, k] on the device, rows by descending window score, equal scores by lower row
        id first; videos without a candidate window come last (start -1, length 0, score -inf), the -1 rows of a short gallery after
        them.
        per_video=P > 1 (at most MOMENT_NBEST_MAX): every video of the shortlist is localised with n_best=P under nms (localize) and
        the shortlist * P moments are ranked -- window score descending, then lower row id, then the earlier pick of a video -- so a
        video may appear up to P times in a row of the result; 1 <= k <= shortlist * P, the shortlist itself (default: k, cut to
        TOPK_MAX) still at most TOPK_MAX.  The empty slots of a video that has fewer than P windows rank with the videos without one."""
        k = int(k)
        if per_video != 1:
            return self._search_moments_nbest(input_ids, token_type_ids, attention_mask, k, window, shortlist, bank, per_video, nms)
        check_nms("VideoIndex.search_moments", nms)
        shortlist = k if shortlist is None else int(shortlist)
        if not 1 <= k <= shortlist <= _lib.TOPK_MAX:
            raise ValueError("VideoIndex.search_moments: k=%d shortlist=%d, need 1 <= k <= shortlist <= %d" % (k, shortlist, _lib.TOPK_MAX))
        if not self.keep_frames:
            raise ValueError("VideoIndex.search_moments needs an index built with keep_frames=True")
        q = self.pool_text(input_ids, token_type_ids, attention_mask)[0]
        _, idx = self.search_vectors(q, shortlist, None, bank)
        start, length, score = self.localize_vectors(q, idx, window)
        sc, order = _rank_rows(score, idx, k)
        return sc, idx.gather(1, order), start.gather(1, order), length.gather(1, order)

    def _search_moments_nbest(self, input_ids, token_type_ids, attention_mask, k, window, shortlist, bank, P, nms):
        who = "VideoIndex.search_moments"
        check_nbest(who, P, nms, "per_video")
        shortlist = min(k, _lib.TOPK_MAX) if shortlist is None else int(shortlist)
        if not (1 <= shortlist <= _lib.TOPK_MAX and 1 <= k <= shortlist * P):
            raise ValueError("%s: k=%d shortlist=%d per_video=%d, need 1 <= shortlist <= %d and 1 <= k <= shortlist * per_video"
                             % (who, k, shortlist, P, _lib.TOPK_MAX))
        if not self.keep_frames:
            raise ValueError("%s needs an index built with keep_frames=True" % who)
        q = self.pool_text(input_ids, token_type_ids, attention_mask)[0]
        _, idx = self.search_vectors(q, shortlist, None, bank)
        start, length, score = (t.flatten(1) for t in self.localize_vectors(q, idx, window, P, nms))
        idx = idx.repeat_interleave(P, dim=1)             # column j * P + m: pick m of shortlist video j; the stable sorts keep m's order
        sc, order = _rank_rows(score, idx, k)
        return sc, idx.gather(1, order), start.gather(1, order), length.gather(1, order)


class QueryBank:
    """A bank of pooled text vectors that normalises the searches of ONE VideoIndex.  With s the index's raw score and b the bank rows,
      c[j]     = log(sum_b exp(beta * s(b, j))) / beta           the column term of gallery row j (ops.sim_colstat)
      hub[j]   = 1 iff j is among the hub_k best rows of some bank row (raw score, ties by lower row id first)
      s'(i, j) = s(i, j) - c[j]  where gate_i is set,  s(i, j)  otherwise
    and gate_i = hub[raw top-1 of query i] (dynamic=True: only queries whose best video is one the bank already claims are
    normalised) or 1 for every query (dynamic=False).  Ranking by s' is ranking by exp(beta s(i, j)) / sum_b exp(beta s(b, j)).
    Fill it with add() / add_vectors(), call fit(), pass it as search(..., bank=).  c[j] depends on gallery row j and the bank alone,
    so fit() after the index grew computes the new rows only and equals a fresh fit() bit for bit; more bank rows recompute all."""

    def __init__(self, index, beta=20.0, hub_k=1, dynamic=True):
        check_bank_args(beta, hub_k)
        self.index, self.beta, self.hub_k, self.dynamic = index, float(beta), int(hub_k), bool(dynamic)
        self._buf, self._n = None, 0
        self._invalidate()

    def _invalidate(self):
        self._covered = 0                     # index rows that c, the lists and hub cover
        self._c = self._top_score = self._top_idx = self._hub = None

    def __len__(self):
        return self._n

    @property
    def vectors(self):
        """[len(bank), 768] fp32 view of the bank rows."""
        return self._buf[:self._n]

    @property
    def c(self):
        """[len(index)] fp32 column terms, as of the last fit() (ValueError before the first, or after more bank rows)."""
        self._need_fit()
        return self._c[:self._covered]

    @property
    def hub(self):
        """[len(index)] int32 hub flags, as of the last fit() (ValueError before the first, or after more bank rows)."""
        self._need_fit()
        return self._hub

    def _need_fit(self):
        if self._c is None:
            raise ValueError("QueryBank: nothing is fitted yet (or the bank changed since); call bank.fit()")

    @torch.no_grad()
    def add(self, input_ids, token_type_ids, attention_mask):
        """Pools the texts as VideoIndex.pool_text does and appends them.  Returns the number of bank rows."""
        return self.add_vectors(self.index.pool_text(input_ids, token_type_ids, attention_mask)[0])

    @torch.no_grad()
    def add_vectors(self, q):
        """Appends pooled vectors the caller already holds ([b, 768] on the index's device).  Invalidates fit()."""
        dev = torch.device(self.index._device())
        if q.device.type != dev.type or (dev.index is not None and q.device.index != dev.index):
            raise ValueError("QueryBank.add_vectors: vectors on %s, the index is on %s" % (q.device, dev))
        q = q.reshape(-1, H)
        b = q.shape[0]
        if b == 0:
            return self._n
        cap = 0 if self._buf is None else self._buf.shape[0]
        if self._n + b > cap:
            self._buf = _grown(self._buf, self._n, max(2 * cap, self._n + b, 64), H, device=q.device)
        self._buf[self._n:self._n + b].copy_(q)
        self._n += b
        self._invalidate()
        return self._n

    @torch.no_grad()
    def fit(self):
        """Column terms and hub flags for the index rows not covered yet (all of them after the bank changed).  Returns self."""
        if self._n == 0:
            raise ValueError("QueryBank.fit: the bank is empty; add() texts first")
        n = len(self.index)
        if n == 0:
            raise ValueError("QueryBank.fit: the index is empty")
        lo = self._covered
        if lo == n:
            return self
        bank, piece = self.vectors, self.index.vectors[lo:n]
        if self._c is None or self._c.numel() < n:
            self._c = _grown(self._c, lo, max(n, self.index._cap), device=bank.device)
        ops.sim_colstat(bank, piece, self.beta, out=self._c[lo:n])
        # every bank row's hub_k best (score, row): the piece's list, merged exactly with the one kept so far (_rank_rows)
        score, idx = ops.sim_topk(bank, piece, self.hub_k)
        idx = torch.where(idx < 0, torch.full_like(idx, _NO_ROW), idx + lo)
        if lo:
            both = torch.cat([self._top_idx, idx], 1)
            score, order = _rank_rows(torch.cat([self._top_score, score], 1), both, self.hub_k)
            idx = both.gather(1, order)
        self._top_score, self._top_idx = score, idx
        self._hub = ops.hub_flags(idx, n)                 # _NO_ROW lies outside every gallery: skipped
        self._covered = n
        return self

    def check_fitted(self, index):
        """ValueError unless fit() covers `index` as it stands."""
        if index is not self.index:
            raise ValueError("QueryBank: this bank belongs to another VideoIndex")
        if self._n == 0 or self._covered != len(index):
            raise ValueError("QueryBank: the bank or the index changed since the last fit (%d of %d index rows covered); call bank.fit()"
                             % (self._covered, len(index)))


_NO_ROW = 2 ** 31 - 1      # an empty slot of a best list (the -1 of ops.sim_topk), made to sort last


def _rank_rows(score, idx, keep=None):
    """THE ranking rule, the kernels' own order: every row of score / idx [rows, n] by descending score, equal scores by lower row id
    first, empty slots (idx < 0 or _NO_ROW) last -- ids ascending, then a stable sort by score.  Returns (sorted scores, order), cut
    to `keep` columns: order[i, j] is the column ranked j-th, to gather idx and its companions with.  Two lists merge by ranking both."""
    ids, perm = torch.sort(torch.where(idx < 0, torch.full_like(idx, _NO_ROW), idx).long(), dim=1, stable=True)
    sc, perm2 = torch.sort(score.gather(1, perm), dim=1, descending=True, stable=True)
    return sc[:, :keep].contiguous(), perm.gather(1, perm2)[:, :keep]


def _query_rows(q):
    """[Nq, 768] fp32 query rows as the kernels read them: copied only where columns are strided or rows not 16-byte aligned."""
    q = q.reshape(-1, H).to(torch.float32)
    return q.contiguous() if q.stride(1) != 1 or q.stride(0) % 4 or q.data_ptr() % 16 else q


def _grown(buf, filled, cap, *shape, device, dtype=torch.float32, zero=False):
    """THE growth of a device row buffer: a new [cap, *shape] one with buf[:filled] copied on the device (buf None: nothing to copy)
    and the rest unspecified, or zero with zero=True.  When to grow and to what capacity is the owner's policy."""
    new = (torch.zeros if zero else torch.empty)(cap, *shape, device=device, dtype=dtype)
    if buf is not None and filled:
        new[:filled].copy_(buf[:filled])
    return new


def check_nms(who, nms):
    """The ValueError of a suppression threshold nms = (num, den), before any device work."""
    ok = isinstance(nms, (tuple, list)) and len(nms) == 2 and all(isinstance(x, numbers.Integral) and not isinstance(x, bool) for x in nms)
    if not ok or not (1 <= nms[1] <= 1024 and 0 <= nms[0] <= nms[1]):
        raise ValueError("%s: nms=%r, need a pair of integers (num, den) with 1 <= den <= 1024 and 0 <= num <= den" % (who, nms))


def check_nbest(who, n_best, nms, name="n_best"):
    """The ValueErrors of (n_best=, nms=), before any device work: n_best None is one window per pair, and then nms must be left alone."""
    if n_best is None:
        if nms is not _NMS:
            raise ValueError("%s: nms=%r without %s; suppression needs more than one window per pair" % (who, nms, name))
        return
    if isinstance(n_best, bool) or not isinstance(n_best, numbers.Integral) or not 1 <= n_best <= _lib.MOMENT_NBEST_MAX:
        raise ValueError("%s: %s=%r, need an integer in [1, %d]" % (who, name, n_best, _lib.MOMENT_NBEST_MAX))
    check_nms(who, nms)


def check_valign_args(who, tau, local, tau_given=True):
    """The ValueErrors of (tau=, local=) of a video alignment, before any device work; tau travels as fp32."""
    if not (isinstance(local, numbers.Integral) and local in (0, 1)):
        raise ValueError("%s: local=%r, need True or False" % (who, local))
    if local and not tau_given:
        raise ValueError("%s: local=True needs an explicit tau (the cosine below which two frames do not match)" % who)
    real = isinstance(tau, numbers.Real) and not isinstance(tau, bool)
    try:
        t32 = ctypes.c_float(tau).value if real else math.nan
    except OverflowError:
        t32 = math.inf
    if not math.isfinite(t32):
        raise ValueError("%s: tau=%r, need a finite fp32 number" % (who, tau))


def check_segment_args(who, switch_penalty, background):
    """The ValueErrors of (switch_penalty=, background=) of a segmentation, before any device work; both travel as fp32."""
    real = lambda x: isinstance(x, numbers.Real) and not isinstance(x, bool)
    p32 = ctypes.c_float(switch_penalty).value if real(switch_penalty) else math.nan
    if not (math.isfinite(p32) and p32 >= 0):
        raise ValueError("%s: switch_penalty=%r, need a finite fp32 number >= 0" % (who, switch_penalty))
    if background is not None:
        b32 = ctypes.c_float(background).value if real(background) else math.nan
        if math.isnan(b32) or b32 == math.inf:
            raise ValueError("%s: background=%r, need a number below +inf in fp32 or -inf (None: no background label)" % (who, background))


def check_bank_args(beta, hub_k):
    """The ValueErrors of QueryBank(beta=, hub_k=), before any device work."""
    ok = isinstance(beta, numbers.Real) and not isinstance(beta, bool)
    b32 = ctypes.c_float(beta).value if ok else 0.0           # beta travels as fp32
    if not (math.isfinite(b32) and b32 > 0):
        raise ValueError("QueryBank: beta=%r, need a finite fp32 number > 0" % (beta,))
    if isinstance(hub_k, bool) or not isinstance(hub_k, numbers.Integral) or not 1 <= hub_k <= _lib.TOPK_MAX:
        raise ValueError("QueryBank: hub_k=%r, need an integer in [1, %d]" % (hub_k, _lib.TOPK_MAX))
