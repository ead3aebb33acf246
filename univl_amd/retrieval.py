"""Retrieval search: build a gallery once, search it many times -- the retrieval counterpart of decode.CaptionBeamSearch.

VideoIndex holds one pooled (and, unless use_mil, L2-normalised) 768-wide fp32 vector per video in ONE device buffer that doubles
when full; a query is pooled the same way get_similarity_logits pools it (modeling.py:377-391) and searched with univl_sim_topk
(include/univl_hip.h): the k best gallery rows per query, sorted by descending score, equal scores by lower row id first, without the
[queries, gallery] matrix.  The opposite direction is the same code: fill an index with text vectors through add_vectors and query it
with video vectors through search_vectors.

Stage-two / train_sim_after_cross models score a pair through the cross encoder; search(..., rerank=True) runs only the k joint-head
candidates of every query through it (queries x k pairs instead of queries x gallery) and re-sorts each row by the cross score."""
import torch

from . import _lib, ops

H = 768


class VideoIndex:
    def __init__(self, model, capacity=1024, keep_frames=False):
        """capacity: rows allocated at first (the buffer doubles when full); keep_frames: also keep every video's visual_output and
        mask, which rerank=True needs."""
        if capacity < 1:
            raise ValueError("VideoIndex: capacity must be at least 1")
        self.model, self.keep_frames = model, bool(keep_frames)
        self._cap, self._n = int(capacity), 0
        self._buf = self._frames = self._fmask = None

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
        dev, cap = self._device(), self._cap
        while self._n + extra > cap:
            cap *= 2
        if self._buf is None or cap != self._cap:
            new = torch.empty(cap, H, device=dev, dtype=torch.float32)
            if self._buf is not None:
                new[:self._n].copy_(self._buf[:self._n])
            self._buf = new
        if self.keep_frames and F is not None:
            if self._frames is not None and self._frames.shape[1] != F:
                raise ValueError("VideoIndex: videos of %d frames in an index of %d-frame videos" % (F, self._frames.shape[1]))
            if self._frames is None or self._frames.shape[0] != cap:
                frames = torch.empty(cap, F, H, device=dev, dtype=torch.float32)
                fmask = torch.zeros(cap, F, device=dev, dtype=torch.int64)
                if self._frames is not None:
                    frames[:self._n].copy_(self._frames[:self._n])
                    fmask[:self._n].copy_(self._fmask[:self._n])
                self._frames, self._fmask = frames, fmask
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
    def search(self, input_ids, token_type_ids, attention_mask, k=10, targets=None, rerank=False, chunk_rows=5):
        """The k best videos for every text.  Returns (scores [Nq, k] fp32, indices [Nq, k] int32) on the device, rows sorted by
        descending score, equal scores by lower row id first, -inf / -1 past the end of a gallery smaller than k.  With targets
        ([Nq] gallery rows) it also returns (gt, eq), the rank counts of every query's target (k = 0: only those).
        rerank=True (keep_frames=True, a model with a cross encoder, k <= len(index)): the k joint-head candidates are scored by
        the cross encoder, chunk_rows queries at a time; returns the cross scores and the re-ordered row ids."""
        q, so, am = self.pool_text(input_ids, token_type_ids, attention_mask)
        if rerank:
            if targets is not None:
                raise ValueError("VideoIndex.search: rank counts are taken from the joint head; call without rerank for them")
            return self._rerank(q, so, am, int(k), int(chunk_rows))
        return self.search_vectors(q, k, targets)

    @torch.no_grad()
    def search_vectors(self, q, k, targets=None):
        """search() for pooled query vectors the caller already holds ([Nq, 768] fp32 on the index's device)."""
        if self._n == 0:
            raise ValueError("VideoIndex: the index is empty")
        q = q.reshape(-1, H).to(torch.float32)
        if q.stride(1) != 1 or q.stride(0) % 4 or q.data_ptr() % 16:
            q = q.contiguous()
        if targets is not None:
            targets = torch.as_tensor(targets).reshape(-1).to(device=q.device, dtype=torch.int32).contiguous()
        return ops.sim_topk(q, self.vectors, int(k), target=targets)

    def _rerank(self, q, so, am, K, chunk_rows):
        from .steps import EvalSession, PoolerSim
        model = self.model
        if model.cross is None:
            raise ValueError("VideoIndex.search(rerank=True): this model has no cross encoder")
        if not self.keep_frames or self._frames is None:
            raise ValueError("VideoIndex.search(rerank=True) needs an index built with keep_frames=True")
        if not 1 <= K <= min(self._n, _lib.TOPK_MAX):
            raise ValueError("VideoIndex.search(rerank=True): k=%d, need 1 <= k <= min(len(index), %d)" % (K, _lib.TOPK_MAX))
        _, idx = ops.sim_topk(q, self.vectors, K)
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
        # each row by descending cross score, equal scores by lower row id first: ids ascending, then a stable sort by score
        ids, perm = torch.sort(idx.long(), dim=1, stable=True)
        sc, perm2 = torch.sort(cross.gather(1, perm), dim=1, descending=True, stable=True)
        return sc, ids.gather(1, perm2).to(torch.int32)
