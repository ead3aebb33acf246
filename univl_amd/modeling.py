"""MI355X-native mirror of the reference's model facade `modules/modeling.py::UniVL`.

Same public surface: `UniVL.from_pretrained()`, `forward()` -> scalar loss,
`get_sequence_visual_output()`, `get_similarity_logits()`, `decoder_caption()`, the attributes the scripts read
(`_stage_one`, `_stage_two`, `train_sim_after_cross`, `task_config`), and the reference's parameter names and
shapes so that `univl.pretrained.bin` / saved checkpoints interchange.  The sub-modules below are PARAMETER
CONTAINERS (their names reproduce the reference's state_dict keys); all arithmetic runs in libunivl_hip.so through
the static plans of `univl_amd.engine` -- there is no PyTorch compute path and no CPU fallback.
"""
import json
import logging
import os
import weakref

import torch
from torch import nn

from . import _ab, _lib, ops
from .engine import FlatParams, Plan
from .optimization import ADOPTED, STARTED
from .parallel import BucketReducer, broadcast_parameters

logger = logging.getLogger(__name__)

# defaults of modules/{visual,cross,decoder}-base/*.json and of BERT-base (module_bert.py:61-72)
BERT_BASE = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                 hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                 max_position_embeddings=512, type_vocab_size=2, initializer_range=0.02)
VISUAL_BASE = dict(BERT_BASE, vocab_size=1024, num_hidden_layers=1)
CROSS_BASE = dict(BERT_BASE, vocab_size=768, num_hidden_layers=2, max_position_embeddings=1024)
DECODER_BASE = dict(BERT_BASE, num_decoder_layers=1, max_target_embeddings=512)


class _Config(object):
    def __init__(self, d):
        self.__dict__.update(d)

    @classmethod
    def resolve(cls, name, defaults, config_file):
        """until_config.py:41-99: a directory holding <config_file> overrides the built-in defaults."""
        d = dict(defaults)
        for cand in (name, os.path.join(os.path.dirname(os.path.abspath(__file__)), str(name))):
            f = os.path.join(str(cand), config_file)
            if os.path.isfile(f):
                with open(f, "r", encoding="utf-8") as r:
                    d.update(json.load(r))
                break
        return cls(d)


def _check_attr(name, cfg):
    return hasattr(cfg, name) and cfg.__dict__[name]


class LayerNorm(nn.Module):
    """Parameter container for until_module.py:40-53 (weight, bias; eps 1e-12)."""

    def __init__(self, hidden_size, eps=1e-12):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.bias = nn.Parameter(torch.zeros(hidden_size))
        self.variance_epsilon = eps


class _SelfAttentionParams(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H)


class _SelfOutputParams(nn.Module):
    def __init__(self, H_in, H):
        super().__init__()
        self.dense = nn.Linear(H_in, H)
        self.LayerNorm = LayerNorm(H)


class _AttentionParams(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.self = _SelfAttentionParams(H)
        self.output = _SelfOutputParams(H, H)


class _IntermediateParams(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.dense = nn.Linear(H, I)


class _LayerParams(nn.Module):
    """BertLayer / VisualLayer / CrossLayer (module_bert.py:253-264)."""

    def __init__(self, H, I):
        super().__init__()
        self.attention = _AttentionParams(H)
        self.intermediate = _IntermediateParams(H, I)
        self.output = _SelfOutputParams(I, H)


class _EncoderParams(nn.Module):
    def __init__(self, H, I, L):
        super().__init__()
        self.layer = nn.ModuleList([_LayerParams(H, I) for _ in range(L)])


class _PoolerParams(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.dense = nn.Linear(H, H)


class _BertEmbeddingsParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.token_type_embeddings = nn.Embedding(cfg.type_vocab_size, cfg.hidden_size)
        self.LayerNorm = LayerNorm(cfg.hidden_size)


class BertModel(nn.Module):
    """Parameters of module_bert.py:364-414."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.embeddings = _BertEmbeddingsParams(cfg)
        self.encoder = _EncoderParams(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers)
        self.pooler = _PoolerParams(cfg.hidden_size)


class _VisualEmbeddingsParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = nn.Linear(cfg.vocab_size, cfg.hidden_size)
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.LayerNorm = LayerNorm(cfg.hidden_size)


class VisualModel(nn.Module):
    """Parameters of module_visual.py:346-395."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.embeddings = _VisualEmbeddingsParams(cfg)
        self.encoder = _EncoderParams(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers)
        self.pooler = _PoolerParams(cfg.hidden_size)


class NormalizeVideo(nn.Module):
    """modeling.py:83-92."""

    def __init__(self, task_config):
        super().__init__()
        self.visual_norm2d = LayerNorm(task_config.video_dim)


class UniVLPreTrainedModel(nn.Module):
    def __init__(self):
        super().__init__()

    @classmethod
    def from_pretrained(cls, pretrained_bert_name, visual_model_name, cross_model_name, decoder_model_name,
                        state_dict=None, cache_dir=None, type_vocab_size=2, *inputs, **kwargs):
        """modeling.py:56-81."""
        task_config = kwargs.get("task_config", None)
        if task_config is not None:
            if not hasattr(task_config, "local_rank"):
                task_config.__dict__["local_rank"] = 0
            elif task_config.local_rank == -1:
                task_config.local_rank = 0
        bert_config = _Config.resolve(pretrained_bert_name, BERT_BASE, "bert_config.json")
        bert_config.type_vocab_size = type_vocab_size
        if state_dict is None and os.path.isfile(os.path.join(str(pretrained_bert_name), "pytorch_model.bin")):
            state_dict = torch.load(os.path.join(str(pretrained_bert_name), "pytorch_model.bin"), map_location="cpu")
        visual_config = _Config.resolve(visual_model_name, VISUAL_BASE, "visual_config.json")
        cross_config = _Config.resolve(cross_model_name, CROSS_BASE, "cross_config.json")
        decoder_config = _Config.resolve(decoder_model_name, DECODER_BASE, "decoder_config.json")
        for c in (visual_config, cross_config, decoder_config):
            c.type_vocab_size = type_vocab_size
        model = cls(bert_config, visual_config, cross_config, decoder_config, *inputs, **kwargs)
        assert model.bert is not None and model.visual is not None
        if state_dict is not None:
            model = cls.init_preweight(model, state_dict, task_config=task_config)
        return model

    @classmethod
    def init_preweight(cls, model, state_dict, prefix=None, task_config=None):
        """until_module.py:91-146: gamma/beta -> weight/bias renames, optional prefix, report missing/unexpected."""
        sd = {}
        for k, v in state_dict.items():
            nk = k.replace("gamma", "weight") if "gamma" in k else k
            nk = nk.replace("beta", "bias") if "beta" in nk else nk
            sd[(prefix + nk) if prefix is not None else nk] = v
        res = model.load_state_dict(sd, strict=False)
        if prefix is None and (task_config is None or task_config.local_rank == 0):
            if res.missing_keys:
                logger.info("Weights of %s not initialized from pretrained model: %s", model.__class__.__name__, res.missing_keys)
            if res.unexpected_keys:
                logger.info("Weights from pretrained model not used in %s: %s", model.__class__.__name__, res.unexpected_keys)
        model.mark_params_dirty()
        return model


class _CrossEmbeddingsParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.token_type_embeddings = nn.Embedding(cfg.type_vocab_size, cfg.hidden_size)
        self.LayerNorm = LayerNorm(cfg.hidden_size)


class CrossModel(nn.Module):
    """Parameters of module_cross.py:356-362."""

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.embeddings = _CrossEmbeddingsParams(cfg)
        self.encoder = _EncoderParams(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers)
        self.pooler = _PoolerParams(cfg.hidden_size)


class _MHAParams(nn.Module):
    def __init__(self, Hd):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(Hd, Hd), nn.Linear(Hd, Hd), nn.Linear(Hd, Hd)


class _DecoderAttentionParams(nn.Module):
    def __init__(self, Hd):
        super().__init__()
        self.att = _MHAParams(Hd)
        self.output = _SelfOutputParams(Hd, Hd)


class _DecoderLayerParams(nn.Module):
    """module_decoder.py:279-285."""

    def __init__(self, Hd, I):
        super().__init__()
        self.slf_attn = _DecoderAttentionParams(Hd)
        self.enc_attn = _DecoderAttentionParams(Hd)
        self.intermediate = _IntermediateParams(Hd, I)
        self.output = _SelfOutputParams(I, Hd)


class _DecoderEmbeddingsParams(nn.Module):
    """module_decoder.py:294-307: word / position tables are BERT's (tied)."""

    def __init__(self, cfg, word_w, pos_w):
        super().__init__()
        self.word_embeddings = nn.Embedding(word_w.shape[0], word_w.shape[1])
        self.position_embeddings = nn.Embedding(pos_w.shape[0], pos_w.shape[1])
        self.word_embeddings.weight = word_w
        self.position_embeddings.weight = pos_w
        self.LayerNorm = LayerNorm(cfg.hidden_size)


class _HeadTransformParams(nn.Module):
    def __init__(self, Hd):
        super().__init__()
        self.dense = nn.Linear(Hd, Hd)
        self.LayerNorm = LayerNorm(Hd)


class _LMPredictionHeadParams(nn.Module):
    """module_bert.py:314-325 / module_decoder.py:170-178: tied decoder.weight + own bias."""

    def __init__(self, Hd, emb_w):
        super().__init__()
        self.transform = _HeadTransformParams(Hd)
        self.decoder = nn.Linear(emb_w.size(1), emb_w.size(0), bias=False)
        self.decoder.weight = emb_w
        self.bias = nn.Parameter(torch.zeros(emb_w.size(0)))


class _OnlyMLMHeadParams(nn.Module):
    def __init__(self, Hd, emb_w):
        super().__init__()
        self.predictions = _LMPredictionHeadParams(Hd, emb_w)


class _VisualLMPredictionHeadParams(nn.Module):
    """module_visual.py:298-306: weight tied to the visual input projection (768,1024), bias (1024)."""

    def __init__(self, Hd, vis_w):
        super().__init__()
        self.transform = _HeadTransformParams(Hd)
        self.weight = vis_w
        self.bias = nn.Parameter(torch.zeros(vis_w.size(1)))


class _VisualOnlyMLMHeadParams(nn.Module):
    def __init__(self, Hd, vis_w):
        super().__init__()
        self.predictions = _VisualLMPredictionHeadParams(Hd, vis_w)


class _DecoderClassifierParams(nn.Module):
    def __init__(self, Hd, emb_w):
        super().__init__()
        self.cls = _OnlyMLMHeadParams(Hd, emb_w)


class _DecoderParams(nn.Module):
    def __init__(self, Hd, I, L):
        super().__init__()
        self.layer = nn.ModuleList([_DecoderLayerParams(Hd, I) for _ in range(L)])


class DecoderModel(nn.Module):
    """Parameters of module_decoder.py:351-370."""

    def __init__(self, cfg, word_w, pos_w):
        super().__init__()
        self.config = cfg
        self.embeddings = _DecoderEmbeddingsParams(cfg, word_w, pos_w)
        self.decoder = _DecoderParams(cfg.hidden_size, cfg.intermediate_size, cfg.num_decoder_layers)
        self.classifier = _DecoderClassifierParams(cfg.hidden_size, word_w)


def _loss_out(step):
    """A fresh 0-d tensor holding the step's loss (the step's own buffer is rewritten by the next forward).  A kernel node,
    not clone(): a device-to-device memcpy is a ~10 us node of the captured step."""
    out = torch.empty((), device=step.loss.device, dtype=step.loss.dtype)
    if out.is_cuda and _ab.get("copy_kernel"):
        from . import ops
        ops.copy_many([(out, step.loss)])
    else:
        out.copy_(step.loss[0])
    return out


class _StepLossFn(torch.autograd.Function):
    """loss = UniVL.forward(...): the whole forward is one static plan, the whole backward another; parameter gradients
    are written straight into the flat gradient buffer (p.grad are views of it)."""

    @staticmethod
    def forward(ctx, anchor, model, step):
        model._run_plan(step.fwd, step)
        ctx.model, ctx.step, ctx.anchor = model, step, anchor
        return _loss_out(step)

    @staticmethod
    def backward(ctx, gout):
        ctx.model._run_backward(ctx.step, gout)
        # Under a stock torch DistributedDataParallel wrapper the anchor is the one parameter DDP still tracks
        # (UniVL._ddp_params_and_buffers_to_ignore lists all others): its autograd hook must fire every iteration.
        ganchor = torch.zeros_like(ctx.anchor) if ctx.model._implicit_dp else None
        return ganchor, None, None


class _LossTensor(torch.Tensor):
    """The scalar returned by UniVL.forward.  It is an ordinary autograd tensor (grad_fn = _StepLossFn), but a plain
    `loss.backward()` -- what main_task_retrieval.py:342 does -- runs the backward plan directly in the calling
    thread instead of going through the autograd engine's device thread (less overhead, and a multi-stream plan can
    then be captured into a hipGraph together with the forward).  Anything else (`(loss / k).backward()`,
    `loss.mean()`, explicit gradients) takes the normal autograd route and ends in _StepLossFn.backward."""

    def __float__(self):
        # `total_loss += float(loss)` (main_task_retrieval.py:344) on a tensor that requires grad: read the detached value
        # (same number, without torch's "converting a tensor with requires_grad=True to a scalar" warning every step)
        a = self.__dict__.get("_async")
        if a is not None:                  # univl_amd.graphed: the value was copied to pinned memory right after the forward;
            a[1].synchronize()             # waiting for THAT copy does not wait for the backward / optimizer behind it
            return float(a[0][0])
        return torch.Tensor.__float__(self.detach())

    def item(self):
        return float(self)

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        ms = self.__dict__.get("_univl", None)
        if ms is not None and gradient is None and inputs is None and not create_graph and not ms[0]._implicit_dp:
            model, step = ms
            model._run_backward(step, None)
            return None
        return super().backward(gradient=gradient, retain_graph=retain_graph, create_graph=create_graph, inputs=inputs)


class UniVL(UniVLPreTrainedModel):
    def __init__(self, bert_config, visual_config, cross_config, decoder_config, task_config):
        super().__init__()
        self.bert_config, self.visual_config = bert_config, visual_config
        self.cross_config, self.decoder_config = cross_config, decoder_config
        self.task_config = task_config
        self.ignore_video_index = -1
        tc = task_config
        assert tc.max_words <= bert_config.max_position_embeddings
        assert tc.max_words <= decoder_config.max_target_embeddings
        assert tc.max_frames <= visual_config.max_position_embeddings
        assert tc.max_words + tc.max_frames <= cross_config.max_position_embeddings
        assert bert_config.hidden_size == 768 and bert_config.num_attention_heads == 12 and \
            bert_config.intermediate_size == 3072, "kernels are specialised for H=768, 12 heads, I=3072"

        self.graph_backward = False
        # operational switches a training process may turn off on the model (UNIVL_AB is refused outside measurement harnesses)
        self.auto_graph = bool(_ab.get("auto_graph"))      # the unchanged loop switches to graph replay on its own
        self.auto_dp = bool(_ab.get("auto_dp"))            # built-in gradient exchange inside an initialised process group
        self.dp_capture = bool(_ab.get("dp_capture"))      # RCCL exchange captured into the step graph (False: host-issued collectives)
        self.auto_ride = _ab.get("adam_ride") != "0"       # optimizer.step() leaves its launch to the next forward (bf16, one process)
        self._operand_pairs = str(_ab.get("pairs"))        # see the `operand_pairs` property
        self._caption_label_smoothing = 0.0                # see the `caption_label_smoothing` property
        self._stage_one, self._stage_two = True, False
        if _check_attr("stage_two", tc):
            self._stage_one, self._stage_two = False, tc.stage_two
        self.train_sim_after_cross = bool(self._stage_one and _check_attr("train_sim_after_cross", tc))

        # modeling.py:133-169 -- same construction order, same conditions
        if hasattr(tc, "text_num_hidden_layers"):
            bert_config.num_hidden_layers = tc.text_num_hidden_layers
        self.bert = BertModel(bert_config)
        word_w = self.bert.embeddings.word_embeddings.weight
        pos_w = self.bert.embeddings.position_embeddings.weight
        if hasattr(tc, "visual_num_hidden_layers"):
            visual_config.num_hidden_layers = tc.visual_num_hidden_layers
        self.visual = VisualModel(visual_config)
        vis_w = self.visual.embeddings.word_embeddings.weight
        self.cross, self.decoder = None, None
        if self._stage_one is False or self.train_sim_after_cross:
            if hasattr(tc, "cross_num_hidden_layers"):
                cross_config.num_hidden_layers = tc.cross_num_hidden_layers
            self.cross = CrossModel(cross_config)
            if self.train_sim_after_cross is False:
                if hasattr(tc, "decoder_num_hidden_layers"):
                    decoder_config.num_decoder_layers = tc.decoder_num_hidden_layers
                self.decoder = DecoderModel(decoder_config, word_w, pos_w)
            if tc.do_pretrain:
                self.cls = _OnlyMLMHeadParams(bert_config.hidden_size, word_w)
                self.cls_visual = _VisualOnlyMLMHeadParams(visual_config.hidden_size, vis_w)
            self.similarity_dense = nn.Linear(bert_config.hidden_size, 1)
        self.normalize_video = NormalizeVideo(tc)
        self.apply(self.init_weights)

        self._flat = None
        self._steps = {}
        self._param_events = {}        # filled by a pipelined optimizer update in flight (univl_amd.graphed)
        self._pending_update = None    # the optimizer that last deferred an update (optimization.BertAdam._defer), if any
        self._rider_update = None      # the optimization.PendingUpdate THIS forward applies (adopted by _adopt_pending_update or by
                                       # graphed.GraphedTrainStep) -- prologue launches + riders of its forward products
        self._in_pipelined_call = False
        self.auto_ride_count = 0       # forwards that applied an update the unchanged loop's optimizer.step() left to them
        self.graph_captures = 0        # captures of plans that can carry an update (_run_plan)
        self._reducer = None
        self._dp_checked, self._implicit_dp = False, False
        self._seed_dev = None
        self._seed = int(getattr(tc, "seed", 42))
        dt = getattr(tc, "compute_dtype", None) or os.environ.get("UNIVL_COMPUTE_DTYPE", "bf16")
        self.compute_dtype = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32,
                              "float32": torch.float32}[str(dt).replace("torch.", "")]
        self.dropout_prob = float(getattr(tc, "dropout_prob", bert_config.hidden_dropout_prob))
        # A stock torch DistributedDataParallel wrapper (main_task_retrieval.py:197-198) must not reduce these
        # gradients a second time: they never pass through autograd's accumulators (the backward plan writes the flat
        # gradient buffer directly and exchanges it itself, see _auto_data_parallel).  DDP reads this list.
        self._ddp_params_and_buffers_to_ignore = self._ddp_ignore_list()

    ANCHOR = "normalize_video.visual_norm2d.bias"

    def _ddp_ignore_list(self):
        names = []
        for mn, m in self.named_modules():
            for pn, _ in list(m.named_parameters(recurse=False)) + list(m.named_buffers(recurse=False)):
                fqn = "%s.%s" % (mn, pn) if mn else pn
                if fqn != self.ANCHOR:
                    names.append(fqn)
        return names

    def _auto_data_parallel(self):
        """First training forward inside an initialised process group with no explicit enable_data_parallel(): the model
        is presumably wrapped the way the reference's scripts wrap it (stock DDP, find_unused_parameters=True).  Turn
        the built-in gradient exchange on, broadcast rank 0's parameters like DDP's constructor does, and route
        loss.backward() through autograd so that DDP's bookkeeping for the anchor parameter stays consistent."""
        self._dp_checked = True
        import torch.distributed as dist
        if not self.auto_dp or not (dist.is_available() and dist.is_initialized()):
            return
        if dist.get_world_size() > 1:
            self.enable_data_parallel()
            self._implicit_dp = True

    # ------------------------------------------------------------------------------------- housekeeping
    def init_weights(self, module):
        """until_module.py:70-85."""
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.bert_config.initializer_range)
        elif isinstance(module, LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    def _apply(self, fn, *a, **kw):
        if self.__dict__.get("_pending_update") is not None:
            self._flush_pending()           # .to() / .float() re-allocate the parameters a pending update still points at
        r = super()._apply(fn, *a, **kw)
        self._flat, self._steps = None, {}      # parameters were re-allocated (e.g. .to(device)): re-flatten lazily
        return r

    def _flush_pending(self):
        """A training step of univl_amd.graphed.GraphedTrainStep(pipeline_optimizer=True) leaves its BertAdam update to be
        applied next to the following forward pass; everything else that reads the parameters applies it first."""
        o = self._pending_update
        if o is not None and not self._in_pipelined_call:
            o.flush()

    def named_parameters(self, *a, **kw):
        """(parameters() goes through here.)  A BertAdam update that optimizer.step() left for the next forward (the unchanged training
        loop, _adopt_pending_update) is applied before anybody is handed the parameters through the module API; the training loop
        itself asks for them only between backward and step (clip_grad_norm_(model.parameters(), ...), main_task_retrieval.py:347),
        where nothing is pending."""
        o = self.__dict__.get("_pending_update")
        if o is not None and o._auto_deferred:
            self._flush_pending()
        return super().named_parameters(*a, **kw)

    def state_dict(self, *a, **kw):
        self._flush_pending()
        fl = self._flat
        if fl is not None and getattr(fl, "shard_reducer", None) is not None and not fl.master_complete:
            raise RuntimeError("UniVL.state_dict(): the fp32 master weights are sharded over the ranks (sharded optimizer) -- "
                               "call model.consolidate_parameters() on EVERY rank first (a collective)")
        return super().state_dict(*a, **kw)

    def train(self, mode=True):
        if not mode:
            self._flush_pending()
        return super().train(mode)

    def mark_params_dirty(self):
        """Tell the model its fp32 parameters were modified outside univl_amd.optimization.BertAdam (the bf16
        shadow the GEMMs read is refreshed before the next forward)."""
        self._flush_pending()               # nothing stays pending across an outside edit (the edit itself should come after a flush:
                                            # INTEGRATION.md, "what a deferred update can and cannot hide")
        if self._flat is not None:
            self._flat.shadow_valid = False

    def load_state_dict(self, *a, **kw):
        self._flush_pending()               #  never on top of the loaded weights
        r = super().load_state_dict(*a, **kw)
        self.mark_params_dirty()
        return r

    def _replicate_for_data_parallel(self):
        self._flush_pending()
        replica = super()._replicate_for_data_parallel()
        replica._flat, replica._steps, replica._reducer, replica._seed_dev = None, {}, None, None
        replica._param_events, replica._pending_update, replica._in_pipelined_call = {}, None, False
        replica._used_names = {}
        replica._dp_checked, replica._implicit_dp, replica.graph_backward = True, False, False
        return replica

    @property
    def flat(self):
        if self._flat is None:
            named = list(self.named_parameters())
            if not named and getattr(self, "_is_replica", False):
                # nn.parallel.replicate (util.py:22, the eval path of main_task_retrieval.py:402-436): a replica's
                # weights are plain tensors kept in _former_parameters; it gets its own flat storage on its device
                seen = set()
                for mn, m in self.named_modules():
                    for k, t in getattr(m, "_former_parameters", {}).items():
                        if t is not None and id(t) not in seen:
                            seen.add(id(t))
                            named.append((("%s.%s" % (mn, k)) if mn else k, t))
            p0 = named[0][1]
            if not p0.is_cuda:
                raise RuntimeError("univl_amd.UniVL runs only on a HIP device (call model.to('cuda')); no CPU fallback")
            _lib.lib()
            if os.environ.get("UNIVL_DETERMINISTIC", "0") == "1" and not _lib.deterministic():
                with torch.cuda.device(p0.device):         # fixed-order reductions (bit-reproducible runs): include/univl_hip.h
                    _lib.set_deterministic(True)
            self._flat = FlatParams(named, p0.device, self.compute_dtype)
            self._flat.owner = weakref.ref(self)
            # forward plans are built with rider slots (engine.Plan.add_gemm_rider: a plain product unless an update rides) wherever a
            # BertAdam update CAN ride with the next forward -- the captured step of graphed.GraphedTrainStep and, round 5, the unchanged
            # training loop (optimization.BertAdam.step defers itself, UniVL.forward applies it: _adopt_pending_update)
            self._flat.adam_ride = self.compute_dtype == torch.bfloat16 and _ab.get("adam_ride") != "0"
            self._flat.operand_pairs = self._operand_pairs
            self._seed_dev = torch.zeros(1, device=p0.device, dtype=torch.int64)
            self._steps = {}
        return self._flat

    @property
    def operand_pairs(self):
        """Precision of the bf16 step's forward products in stacks of at most 768 tokens (16 pairs x 48): '' (default) plain bf16 MFMA
        operands; 'x' / 'w' / 'xw': the activation / weight / both operands as PAIRS of bf16 (hi + lo = 16 mantissa bits,
        include/univl_hip.h: UnivlGemm.A_lo / B_lo).  'xw' brings the median per-tensor gradient error against the reference's fp32
        gradients from 9e-3 to 5.6e-3 and the pretrain configuration's global error from 1.2e-2 to 7.3e-3, at +22 % step time at
        4 pairs per GPU (DESIGN.md section 2 has the table) -- which is why it is a choice and not the default.  Setting it rebuilds
        the plans on the next forward."""
        return self._operand_pairs

    @operand_pairs.setter
    def operand_pairs(self, value):
        value = "" if value is None else str(value)
        if value not in ("", "x", "w", "xw"):
            raise ValueError("operand_pairs: '', 'x', 'w' or 'xw' (got %r)" % (value,))
        if value != self._operand_pairs:
            self._flush_pending()
            self._operand_pairs = value
            if self._flat is not None:
                self._flat.operand_pairs = value
                self._steps = {}

    SMOOTHED_KINDS = ("caption", "caption_weighted", "pretrain")      # the step kinds whose decoder loss takes caption_label_smoothing

    @property
    def caption_label_smoothing(self):
        """Label smoothing eps of the caption decoder's cross entropy (torch.nn.CrossEntropyLoss(label_smoothing=eps); no counterpart in
        the reference, which trains on hard targets): 0.0 (default) or 0 < eps < 1.  It applies to the training loss of the `caption`,
        `caption_weighted` and `pretrain` steps -- in `pretrain` to the decoder term only, never to the MLM head -- through the smoothed
        form of K16 (include/univl_hip.h: univl_vocab_ce_smooth_fwd / _bwd); at 0 the plans are the unsmoothed ones, launch for launch.
        eval.eval_caption_loss and score.CaptionScorer report the unsmoothed likelihood whatever this is.  Setting it rebuilds the plans
        on the next forward."""
        return self._caption_label_smoothing

    @caption_label_smoothing.setter
    def caption_label_smoothing(self, value):
        try:
            value = float(value)
        except (TypeError, ValueError):
            raise ValueError("caption_label_smoothing: a number with 0 <= eps < 1 (got %r)" % (value,)) from None
        if not 0.0 <= value < 1.0:                         # NaN fails both comparisons
            raise ValueError("caption_label_smoothing: 0 <= eps < 1 (got %r)" % (value,))
        if value != self._caption_label_smoothing:
            self._flush_pending()
            self._caption_label_smoothing = value
            if self._flat is not None:
                self._steps = {}

    def enable_data_parallel(self, process_group=None, broadcast=True, loopback=False, force=False, shard_optimizer=None):
        """Re-homes the reference's DDP wrap (main_task_retrieval.py:197-198) onto per-layer RCCL all-reduces of
        the flat gradient buffer, overlapped with backward (univl_amd.parallel).  Call after model.to(device) and
        torch.distributed.init_process_group; with world_size 1 it is a no-op."""
        fl = self.flat
        self._dp_checked, self._implicit_dp = True, False
        if broadcast:
            broadcast_parameters(fl.p32, 0, process_group)
            fl.shadow_valid = False
        self._reducer = BucketReducer(fl.g32, process_group, loopback=loopback, force=force)
        if not self._reducer.active:
            self._reducer = None
        elif self.dp_capture and not loopback and fl.device.type == "cuda":
            # RCCL: a communicator of our own, so that the exchange is captured into the step's hipGraph (univl_amd.rccl)
            try:
                with torch.cuda.device(fl.device):
                    self._reducer.enable_capture()
            except Exception as ex:      # noqa: BLE001 -- the process-group path below does the same exchange from the host
                import sys
                print("[univl_amd] RCCL communicator for captured gradient exchange unavailable (%s: %s); using torch.distributed "
                      "collectives between captured segments" % (type(ex).__name__, ex), file=sys.stderr)
        fl.owned, fl.shard_reducer, fl.master_complete = None, None, True
        fl.partition_version = getattr(fl, "partition_version", 0) + 1      # chunk-table caches of the optimizer are keyed on it
        if shard_optimizer is None:
            shard_optimizer = os.environ.get("UNIVL_SHARD_OPT", "0") == "1"
        if shard_optimizer and self._reducer is not None and not loopback:
            # reduce-scatter of the gradients, clip + BertAdam on this rank's 1/world of every bucket, all-gather of the
            # bf16 shadow (univl_amd.parallel).  The fp32 master and the moments of the other ranks' pieces go stale on this
            # rank: consolidate_parameters() / optimizer.consolidate() (collectives) bring them together for a checkpoint.
            from .parallel import shard_partition
            self._reducer.set_partition(shard_partition(fl, self._reducer.world))
            fl.owned, fl.shard_reducer = self._reducer.owned, self._reducer
        self._steps = {}
        return self

    def consolidate_parameters(self):
        """Sharded optimizer: COLLECTIVE (every rank calls it) -- gathers every rank's pieces of the fp32 master weights, after
        which state_dict() is complete on every rank."""
        fl = self.flat
        red = getattr(fl, "shard_reducer", None)
        if red is not None and not fl.master_complete:
            self._flush_pending()
            red.join()
            red.all_gather_ranges(fl.p32)
            red.join()
            fl.master_complete = True
        return self

    def step_kind(self, has_caption):
        """Which of the reference's forward() branches applies (modeling.py:204-267)."""
        tc = self.task_config
        if self._stage_one:
            return "align" if self.train_sim_after_cross else "joint"
        if tc.do_pretrain:
            return "pretrain" if has_caption else "pretrain_nocap"     # modeling.py:238: the decoder loss needs captions
        if tc.task_type == "caption":
            return "caption"
        return "align"                       # stage two, task_type "retrieval": cross-encoder similarity + CrossEn

    def used_parameter_names(self, kind=None):
        """Parameters that receive a gradient in this configuration (the reference leaves `.grad = None` on the rest:
        dead poolers modeling.py:307,310; the cross pooler / similarity_dense on the caption path)."""
        kind = kind or self.step_kind(True)
        cached = self.__dict__.setdefault("_used_names", {}).get(kind)
        if cached is not None:
            return cached
        out = self._used_names[kind] = []
        for n, _ in self.named_parameters():
            if n.startswith("bert.pooler") or n.startswith("visual.pooler"):
                continue
            if kind in ("caption", "caption_weighted") and (n.startswith("cross.pooler") or n.startswith("similarity_dense")):
                continue
            if kind == "align" and (n.startswith("decoder.") or n.startswith("cls")):
                continue
            if kind == "pretrain_nocap" and n.startswith("decoder."):
                continue
            out.append(n)
        return out

    # ---------------------------------------------------------------------------------------- execution
    def _step_key(self, kind, B, W, F, n_cand=1, Wd=None):
        """n_cand, Wd: part of a "caption_weighted" step's signature only.  A non-zero caption_label_smoothing is the last element of the
        key of the kinds it applies to; at 0 the keys are the ones they were without the property."""
        key = (kind, B, W, F, self.training) + ((n_cand, Wd) if kind == "caption_weighted" else ())
        if kind in self.SMOOTHED_KINDS and self._caption_label_smoothing > 0:
            key += (("smoothing", self._caption_label_smoothing),)
        return key

    def _get_step(self, kind, B, W, F, n_cand=1, Wd=None):
        """n_cand, Wd: the captions per video and their positions, part of a "caption_weighted" step's signature only."""
        key = self._step_key(kind, B, W, F, n_cand, Wd)
        st = self._steps.get(key)
        if st is None:
            from .steps import build_step
            st = build_step(self, kind, B, W, F, self.training, n_cand=n_cand, Wd=Wd)
            self._steps[key] = st
        return st

    def dropout_offsets(self):
        """{step key: {site name: dropout stream offset}} of the training steps built so far (steps.dropout_offsets): what a test needs,
        with self._seed and self._seed_dev, to rebuild every dropout mask of a step on the host.  Read-only."""
        from .steps import Step, dropout_offsets
        return {key: dropout_offsets(st) for key, st in self._steps.items() if isinstance(st, Step) and st.cx.training}

    def dropout_host_seeds(self):
        """{step key: {site name: host seed}}: the seed each site's kernels add the device word self._seed_dev to (self._seed at the
        embedding sites, 0 in the layer stacks -- steps._dropout_sites).  Read-only."""
        from .steps import Step, dropout_host_seeds
        return {key: dropout_host_seeds(st) for key, st in self._steps.items() if isinstance(st, Step) and st.cx.training}

    def _caption_weighted_shape(self,B, input_caption_ids, decoder_mask, output_caption_ids, caption_weight):
        """forward(caption_weight=...): (n_cand, Wd) of a reward-weighted caption batch, or ValueError -- host-side checks on shapes and
        on the model's configuration only, before any device work."""
        if self.decoder is None:
            raise ValueError("UniVL.forward: caption_weight given, but this model was built without a decoder (stage one)")
        if self.step_kind(True) != "caption":
            raise ValueError("UniVL.forward: caption_weight is supported in stage-two caption mode only (stage_two with task_type "
                             "'caption', no do_pretrain); this model's forward is %r" % (self.step_kind(True),))
        if any(t is None for t in (input_caption_ids, decoder_mask, output_caption_ids)):
            raise ValueError("UniVL.forward: caption_weight needs input_caption_ids, decoder_mask and output_caption_ids")
        if caption_weight.dim() != 2 or caption_weight.shape[0] != B or caption_weight.shape[1] < 1:
            raise ValueError("UniVL.forward: caption_weight of shape %s, expected [%d, n_cand] with n_cand >= 1 (one row per video)"
                             % (tuple(caption_weight.shape), B))
        n_cand = int(caption_weight.shape[1])
        Wd = int(input_caption_ids.shape[-1])
        for name, t in (("input_caption_ids", input_caption_ids), ("decoder_mask", decoder_mask), ("output_caption_ids", output_caption_ids)):
            if tuple(t.shape) != (B, n_cand, Wd):
                raise ValueError("UniVL.forward: %s of shape %s, expected [%d, %d, %d] (videos, captions per video as in caption_weight, "
                                 "positions)" % (name, tuple(t.shape), B, n_cand, Wd))
        if not 1 <= Wd <= self.decoder_config.max_target_embeddings:
            raise ValueError("UniVL.forward: captions of %d positions, expected 1 .. %d" % (Wd, self.decoder_config.max_target_embeddings))
        return n_cand, Wd

    AUTO_GRAPH_AFTER = 2
    GRAPH_SIGS = 4

    def _run_plan(self, plan, st):
        """Enqueue a forward / backward plan.  Launched kernel by kernel from Python the host is the bottleneck at small
        batch (~10 us per launch against 2-10 us kernels), so once a step signature has been run AUTO_GRAPH_AFTER times
        eagerly its plans are captured into hipGraphs (engine.Plan.run_graphed: one graph, or captured segments around
        host-issued collectives) and replayed from then on -- the unchanged training loop of main_task_retrieval.py:333-352
        then runs close to the fully captured step of graphed.GraphedTrainStep.  UNIVL_AUTO_GRAPH=0 turns it off; inside
        somebody else's capture the plan is always enqueued directly."""
        hot = self.auto_graph and st.calls > self.AUTO_GRAPH_AFTER
        if (self.graph_backward or hot) and not torch.cuda.is_current_stream_capturing():
            if plan.rider_keys:
                # a captured plan holds the riding update's descriptor and chunk ranges: replay only while they are the ones captured
                # (steady state of a training loop: same optimizer tables, same buffers, so "no riders" + one update descriptor),
                # else capture again
                sig = None if plan.riders is None else plan.riders.signature()
                if plan.select_segments(sig, self.GRAPH_SIGS):
                    self.graph_captures += 1
                    if sig is not None:
                        import ctypes as C              # the rider kernels' large-LDS opt-in must not happen inside the capture
                        _lib.check(_lib.lib().univl_gemm_rider_prime(C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gemm_rider_prime")
            plan.run_graphed()
        else:
            plan.run()

    def _run_backward(self, st, gout):
        fl = self.flat
        used = self.used_parameter_names(st.kind)
        fresh = all(fl.params[n].grad is None for n in (used[0], used[-1]))
        if gout is not None:                 # st.gout holds 1.0 between backwards (steps.Step): plain loss.backward() writes nothing
            st.gout.copy_(gout.reshape(1).to(torch.float32))
        if fl._pending is not None:          # a deferred clip nobody consumed: it scales the OLD gradients, as torch's did
            from .optimization import apply_pending_clip
            apply_pending_clip(fl)
        if fl.g32._version != getattr(fl, "_g32_tv", fl.g32._version):
            fl.mark_all_word_rows()          # the gradients were edited through torch since the last backward: rows unknown
            if getattr(fl, "_word_rows", None) is not None:
                fl._word_rows[1][1] = 1
        fl.grad_version += 1
        self._run_plan(st.backward_plan(fresh), st)
        plan = st.backward_plan(fresh)
        fl.fused = (dict(version=fl.grad_version, names=plan.fused_names, tv=fl.g32._version)
                    if plan.fused_names else None)
        fl._g32_tv = fl.g32._version
        if getattr(plan, "rows_mode", False):
            fl.word_rows_version = fl.grad_version            # the row list describes exactly these gradients
        else:
            fl.mark_all_word_rows()                            # a writer that lists no rows (tied heads, token gather above the cap)
            if getattr(fl, "_word_rows", None) is not None:
                fl._word_rows[1][1] = 1                        # a dense writer ran: every row counts as listed from now on
        fl.attach_grads(used)
        if gout is not None:
            st.gout.fill_(1.0)

    def forward(self, input_ids, token_type_ids, attention_mask, video, video_mask=None,
                pairs_masked_text=None, pairs_token_labels=None, masked_video=None, video_labels_index=None,
                input_caption_ids=None, decoder_mask=None, output_caption_ids=None, caption_weight=None):
        """modeling.py:188-271.  Returns the scalar loss in training mode, None otherwise.
        caption_weight [B, n_cand] (no counterpart in the reference): reward-weighted caption training.  The caption tensors are then
        [B, n_cand, Wd] -- n_cand captions per video -- and the loss is sum_r w_r nll_r / n_valid over all their counting positions, w_r
        the weight of the caption position r belongs to (the "caption_weighted" step, steps.build_step).  Single process only."""
        if not self.training:
            return None
        W, F = input_ids.shape[-1], video_mask.shape[-1]
        B = input_ids.numel() // W
        kind = self.step_kind(input_caption_ids is not None)
        n_cand, Wd = 1, None
        if caption_weight is not None:
            n_cand, Wd = self._caption_weighted_shape(B, input_caption_ids, decoder_mask, output_caption_ids, caption_weight)
            kind = "caption_weighted"
        if kind == "caption" and input_caption_ids is None:
            # modeling.py:238-254: without captions the caption task has no loss term at all (the reference returns the
            # float 0.0, whose .backward() fails in the script)
            raise RuntimeError("UniVL.forward: the caption path needs input_caption_ids / decoder_mask / output_caption_ids")
        if not self._dp_checked:
            self._auto_data_parallel()
        if kind == "caption_weighted" and (self._reducer is not None or getattr(self._flat, "shard_reducer", None) is not None):
            raise NotImplementedError("UniVL.forward(caption_weight=...): the weighted caption step is single-process only; data parallel "
                                      "and the sharded optimizer are not supported for it")
        st, own = None, self._rider_update is None      # own: an update this forward applies is one it adopted itself
        try:
            self._adopt_pending_update()
            upd = self._rider_update               # the update THIS forward applies: adopted just now, or by graphed.GraphedTrainStep
            if upd is None:
                self._flush_pending()
            fl = self.flat
            if getattr(fl, "shard_reducer", None) is not None:
                fl.shard_reducer.join()            # the all-gather of the updated shadow must have landed
            fl.refresh_shadow()
            st = self._get_step(kind, B, W, F, n_cand, Wd)
            st.enc.load(input_ids, token_type_ids, attention_mask, video, video_mask)
            if kind in ("pretrain", "pretrain_nocap"):
                st.enc_m.load(pairs_masked_text, token_type_ids, attention_mask, masked_video, video_mask)
                st.heads.load(pairs_token_labels, video_labels_index)
            if st.decoder is not None:
                st.decoder.load(input_caption_ids, decoder_mask, output_caption_ids, caption_weight)
            anchor = fl.params[self.ANCHOR]
            st.calls += 1
            if upd is not None:
                st.fwd.riders = upd.start(st.fwd.rider_keys)
            if torch.is_grad_enabled() and anchor.requires_grad:
                out = _StepLossFn.apply(anchor, self, st).as_subclass(_LossTensor)
                out._univl = (self, st)
            else:
                self._run_plan(st.fwd, st)
                out = _loss_out(st)
            if upd is not None:
                upd.done()
            return out
        except BaseException as ex:
            # an update this forward took is never left behind or half applied in silence (optimization.PendingUpdate).  Nothing of it
            # launched yet (a bad batch shape, out of memory while a new step was built, a failing join): handed back, pending again,
            # the next forward or any flush applies it once.  Started: what has not gone out goes out now, or RuntimeError(PARTIAL).
            # An update graphed.GraphedTrainStep adopted keeps that object's rule: the capture it failed in never ran, the prepared
            # update is dropped with it (has_pending stays False) and the next call prepares a new one.
            upd = self._rider_update if own else None
            if upd is not None and upd.state == ADOPTED:
                upd.hand_back()
            elif upd is not None and upd.state == STARTED:
                upd.complete_after_failure(None if st is None else st.fwd.riders, ex)
            raise
        finally:
            if st is not None:
                st.fwd.riders = None
            self._rider_update = None

    def _adopt_pending_update(self):
        """The unchanged training loop (main_task_retrieval.py:333-353): optimizer.step() left its BertAdam update pending
        (optimization.BertAdam.step: auto-deferred), and THIS forward applies it -- the chunk groups the plan cannot carry as launches in
        front of it, the rest as extra workgroups of its own products (optimization.PendingUpdate.start) -- exactly what the captured
        step of graphed.GraphedTrainStep does.  Anything else that reads the parameters flushes the update first (_flush_pending)."""
        o = self._pending_update
        if o is None or self._in_pipelined_call or self._rider_update is not None or not o._auto_deferred:
            return
        fl = self.flat
        if not fl.adam_ride or getattr(fl, "shard_reducer", None) is not None or torch.cuda.is_current_stream_capturing():
            return
        # fl.shadow_valid is left as it is: the update rewrites the bf16 shadow of the tensors it updates, and a shadow that was marked
        # dirty (mark_params_dirty, a broadcast) is still refreshed from the fp32 master by this forward, in front of the riders
        self._rider_update = o._update.adopt(max_blocks=0)

    def get_sequence_visual_output(self, input_ids, token_type_ids, attention_mask, video, video_mask, shaped=False):
        """modeling.py:299-313.  `shaped=True` means the caller already flattened the pair dim AND normalised the video
        (only UniVL.forward does that in the reference); external callers use shaped=False."""
        W, F = input_ids.shape[-1], video_mask.shape[-1]
        B = input_ids.numel() // W
        self._flush_pending()
        fl = self.flat
        fl.refresh_shadow()
        was = self.training
        self.training = False                      # feature extraction never applies dropout plans' training variant
        try:
            # shaped=True (modeling.py:300-305 skipped): `video` is already float32 [B, F, video_dim] and normalised
            st = self._get_step("features_shaped" if shaped else ("joint" if self.cross is None else "features"), B, W, F)
        finally:
            self.training = was
        st.enc.load(input_ids, token_type_ids, attention_mask, video, video_mask)
        st.fwd.run(upto=st.fwd_encoders_len)
        return st.enc.seq_out.view(B, W, -1).clone(), st.enc.vis_out.view(B, F, -1).clone()

    def _single_branch_step(self, kind, B, W, F):
        """Flushes a pending optimizer update and refreshes the shadow exactly as get_sequence_visual_output does, then hands
        out the eval-mode plan that builds ONE encoder stack (steps.EncoderPass(branches=...))."""
        self._flush_pending()
        self.flat.refresh_shadow()
        was = self.training
        self.training = False
        try:
            return self._get_step(kind, B, W, F)
        finally:
            self.training = was

    def get_visual_output(self, video, video_mask, shaped=False):
        """The video half of get_sequence_visual_output (modeling.py:299-313) alone: NormalizeVideo + VisualModel, the text stack
        is neither built nor run.  Eval-only; `shaped` as there.  Returns [B, F, 768] fp32."""
        F = video_mask.shape[-1]
        B = video_mask.numel() // F
        st = self._single_branch_step("features_vis_shaped" if shaped else "features_vis", B, 0, F)
        st.enc.load_video(video, video_mask)
        st.fwd.run(upto=st.fwd_encoders_len)
        return st.enc.vis_out.view(B, F, -1).clone()

    def get_sequence_output(self, input_ids, token_type_ids, attention_mask, shaped=False):
        """The text half of get_sequence_visual_output alone: BertModel, the video stack is neither built nor run.  Eval-only;
        `shaped` only says that the pair dimension is already flattened, which the reshape below does not need to know.
        Returns [B, W, 768] fp32."""
        W = input_ids.shape[-1]
        B = input_ids.numel() // W
        st = self._single_branch_step("features_text", B, W, 0)
        st.enc.load_text(input_ids, token_type_ids, attention_mask)
        st.fwd.run(upto=st.fwd_encoders_len)
        return st.enc.seq_out.view(B, W, -1).clone()

    def get_similarity_logits(self, sequence_output, visual_output, attention_mask, video_mask, shaped=False,
                              _pretrain_joint=False):
        """modeling.py:377-391: cross-encoder similarity when stage two / train_sim_after_cross, else masked means,
        L2 normalisation unless use_mil, text . video^T."""
        attention_mask = attention_mask.reshape(-1, attention_mask.shape[-1])
        video_mask = video_mask.reshape(-1, video_mask.shape[-1])
        _lib.lib()
        dev = sequence_output.device
        if dev.type != "cuda":
            raise RuntimeError("univl_amd.UniVL.get_similarity_logits needs HIP device tensors; no CPU fallback")
        Bt, W, Hd = sequence_output.shape
        Bv, F, _ = visual_output.shape
        seq = sequence_output.to(torch.float32).contiguous()
        vis = visual_output.to(torch.float32).contiguous()
        am = attention_mask.to(dev, torch.int64).contiguous()
        vm = video_mask.to(dev, torch.int64).contiguous()
        if (self._stage_two and _pretrain_joint is False) or self.train_sim_after_cross:
            return self._cross_similarity_eval(seq, vis, am, vm)
        norm = not bool(self.task_config.use_mil)
        ldt, ldv = (Bt + 3) // 4 * 4, (Bv + 3) // 4 * 4
        tn = torch.zeros(ldt, Hd, device=dev)
        vn = torch.zeros(ldv, Hd, device=dev)
        ops.pool_fwd(Bt, W, seq, am, skip_first=True, normalize=norm, out=tn)
        ops.pool_fwd(Bv, F, vis, vm, skip_first=False, normalize=norm, out=vn)
        sim = torch.empty(Bt, Bv, device=dev)
        ops.gemm(tn, vn, Bt, Bv, Hd, out32=sim)
        return sim

    def _eval_session(self, key, build):
        """The steps.EvalSession cached under `key` in self._steps (build() makes it on first use), behind the flush of a pending optimizer
        update and the shadow refresh that every reader of the parameters starts with."""
        self._flush_pending()
        self.flat.refresh_shadow()
        ses = self._steps.get(key)
        if ses is None:
            ses = self._steps[key] = build()
        return ses

    def _cross_similarity_eval(self, seq, vis, am, vm, chunk_rows=5):
        """_cross_similarity (modeling.py:341-375) for cached features: every (text, video) pair through the cross
        encoder, `chunk_rows` text rows at a time (the reference's step_size = 5)."""
        from .steps import EvalSession, PoolerSim
        Bt, W, _ = seq.shape
        Bv, F, _ = vis.shape
        out = torch.empty(Bt, Bv, device=seq.device)
        for lo in range(0, Bt, chunk_rows):
            n = min(chunk_rows, Bt - lo)
            ses = self._eval_session(("xsim", n, Bv, W, F), lambda: EvalSession(
                self, n, Bv, W, F, [i for i in range(n) for _ in range(Bv)], list(range(Bv)) * n, PoolerSim, n, Bv, None))
            ses.feats.load(seq[lo:lo + n], vis, am[lo:lo + n], vm)
            ses.plan.run()
            out[lo:lo + n].copy_(ses.head.sim.view(n, Bv))
        return out

    def decoder_caption(self, sequence_output, visual_output, input_ids, attention_mask, video_mask, input_caption_ids,
                        decoder_mask, shaped=False, get_logits=False):
        """modeling.py:409-428: cross encoder on cat(text, video) then the decoder; returns the (n, len, vocab) logits or
        their argmax."""
        if self.decoder is None:
            raise RuntimeError("decoder_caption: this model was built without a decoder (stage one)")
        from .steps import DecoderRun, EvalSession
        attention_mask = attention_mask.reshape(-1, attention_mask.shape[-1])
        video_mask = video_mask.reshape(-1, video_mask.shape[-1])
        input_caption_ids = input_caption_ids.reshape(-1, input_caption_ids.shape[-1])
        decoder_mask = decoder_mask.reshape(-1, decoder_mask.shape[-1])
        B, W, _ = sequence_output.shape
        F, Wd = visual_output.shape[1], input_caption_ids.shape[-1]
        if sequence_output.device.type != "cuda":
            raise RuntimeError("univl_amd.UniVL.decoder_caption needs HIP device tensors; no CPU fallback")
        ses = self._eval_session(("caption_eval", B, W, F, Wd), lambda: EvalSession(
            self, B, B, W, F, list(range(B)), list(range(B)), DecoderRun, Wd, False))
        dec = ses.head
        ses.feats.load(sequence_output.to(torch.float32), visual_output.to(torch.float32), attention_mask, video_mask)
        dec.load(input_caption_ids, decoder_mask)
        ses.plan.run()
        V = self.bert_config.vocab_size
        scores = dec.head.logits.view(B, Wd, -1)[:, :, :V]
        if get_logits:
            return scores.clone()
        return torch.max(scores, -1)[1]
