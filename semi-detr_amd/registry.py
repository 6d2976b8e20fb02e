"""Registration under the reference's plugin names, for trees where mmcv / mmdet are installed.

The reference instantiates everything through mmcv registries and ``type=`` strings in its configs
(``@BBOX_ASSIGNERS.register_module()`` hungarian_assigner.py:16, o2m_assigner.py:17, ``@MATCH_COST.register_module()``
match_cost.py:8,53,146, ``@HOOKS.register_module()`` mean_teacher.py:7).  ``register_all(force=True)``
replaces those entries with the gfx950 implementations so ``configs/dino_detr`` and ``configs/detr_ssod``
run unchanged.  mmcv/mmdet are NOT installed in the build image, so this module only does something where
they exist; importing it elsewhere is harmless (returns the list of names it could not register).
"""


def register_all(force=True, positional_encoding=None):
    from .matcher import BBoxL1Cost, FocalLossCost, HungarianAssigner, IoUCost, O2MAssigner
    from .mean_teacher import MeanTeacher

    done, skipped = [], []
    try:
        from mmdet.core.bbox.builder import BBOX_ASSIGNERS
        from mmdet.core.bbox.match_costs.builder import MATCH_COST
        BBOX_ASSIGNERS.register_module(name="HungarianAssigner", force=force, module=HungarianAssigner)
        BBOX_ASSIGNERS.register_module(name="O2MAssigner", force=force, module=O2MAssigner)
        for cls in (BBoxL1Cost, FocalLossCost, IoUCost):
            MATCH_COST.register_module(name=cls.__name__, force=force, module=cls)
        done += ["HungarianAssigner", "O2MAssigner", "BBoxL1Cost", "FocalLossCost", "IoUCost"]
    except ImportError:
        skipped += ["HungarianAssigner", "O2MAssigner", "BBoxL1Cost", "FocalLossCost", "IoUCost"]
    try:
        from mmdet.models.builder import LOSSES
        from .losses import TaskAlignedFocalLoss
        LOSSES.register_module(name="TaskAlignedFocalLoss", force=force, module=TaskAlignedFocalLoss)
        done.append("TaskAlignedFocalLoss")
    except ImportError:
        skipped.append("TaskAlignedFocalLoss")
    try:
        from mmcv.runner.hooks import HOOKS
        HOOKS.register_module(name="MeanTeacher", force=force, module=MeanTeacher)
        done.append("MeanTeacher")
    except ImportError:
        skipped.append("MeanTeacher")
    try:       # so that mmcv's is_module_wrapper() (runner, hooks, checkpoint code) unwraps the DDP replacement
        from mmcv.parallel import MODULE_WRAPPERS
        from .dp import FlatDDP
        MODULE_WRAPPERS.register_module(name="FlatDDP", force=force, module=FlatDDP)
        done.append("FlatDDP")
    except ImportError:
        skipped.append("FlatDDP")
    # the pyramid's positional encoding under the reference's name (positional_encoding.py:9), where a registry is given or
    # mmcv's is importable; without either there is nothing to report
    if positional_encoding is None:
        try:
            from mmcv.cnn.bricks.transformer import POSITIONAL_ENCODING as positional_encoding
        except ImportError:
            positional_encoding = None
    if positional_encoding is not None:
        from .pyramid_inputs import SinePositionalEncodingHW
        positional_encoding.register_module(name="SinePositionalEncodingHW", force=force, module=SinePositionalEncodingHW)
        done.append("SinePositionalEncodingHW")
    return done, skipped


def register_losses(force=True):
    """``FocalLoss`` under mmdet's ``LOSSES`` (configs name it as ``loss_cls2``, dino_detr_ssod_r50_coco_120k.py:36-41):
    the mmcv-full op it calls on GPU tensors is not part of this stack.  Separate from ``register_all`` so that callers
    opt in.  Returns (registered, skipped) names."""
    try:
        from mmdet.models.builder import LOSSES
        from .set_loss import FocalLoss
        LOSSES.register_module(name="FocalLoss", force=force, module=FocalLoss)
        return ["FocalLoss"], []
    except ImportError:
        return [], ["FocalLoss"]


def bind_dn_queries():
    """Rebind the reference's query builders to ``semi_detr_amd.dn_query`` where ``detr_od`` / ``detr_ssod`` are importable:
    ``prepare_for_cdn`` as the supervised head's module global (dino_detr_head.py:1032), ``prepare_for_cdn_plus`` as the SSOD
    head's (dino_detr_ssod_head.py:1263; both call them by bare name, so the importing module's attribute is what counts,
    and dn_components' own is replaced too) and ``DinoDetrSSOD.prepare_unsup_cdn``.  Returns (bound, skipped) names."""
    import importlib

    from . import dn_query
    done, skipped = [], []
    for mod, name in (("detr_od.models.dense_heads.dino_detr_head", "prepare_for_cdn"),
                      ("detr_od.models.dense_heads.dino_detr_ssod_head", "prepare_for_cdn_plus")):
        try:
            m = importlib.import_module(mod)
            setattr(m, name, getattr(dn_query, name))
            comp = importlib.import_module("detr_od.models.dense_heads.dn_components")
            setattr(comp, name, getattr(dn_query, name))
            done.append(name)
        except ImportError:
            skipped.append(name)
    try:
        m = importlib.import_module("detr_ssod.models.dino_detr_ssod")
        m.DinoDetrSSOD.prepare_unsup_cdn = dn_query.prepare_unsup_cdn
        done.append("DinoDetrSSOD.prepare_unsup_cdn")
    except ImportError:
        skipped.append("DinoDetrSSOD.prepare_unsup_cdn")
    return done, skipped


def bind_query_select():
    """Bind the two-stage query selection to ``semi_detr_amd.query_select`` where ``detr_od`` is importable:
    ``gen_encoder_output_proposals`` as the module global of detr_od.models.utils.transformer (``DINOTransformer.forward`` calls
    it by bare name, transformer.py:1318) and ``DINOTransformer.two_stage_queries`` as a helper method (INTEGRATION.md shows the
    call that replaces transformer.py:1315-1346 and 1394-1398).  Returns (bound, skipped) names."""
    import importlib

    from . import query_select
    names = ["gen_encoder_output_proposals", "DINOTransformer.two_stage_queries"]
    try:
        m = importlib.import_module("detr_od.models.utils.transformer")
    except ImportError:
        return [], names
    m.gen_encoder_output_proposals = query_select.gen_encoder_output_proposals
    m.DINOTransformer.two_stage_queries = query_select.two_stage_queries
    return names, []


def bind_decoder_self_attention():
    """Where ``detr_od`` is importable, wrap the decoder layer's ``__init__`` (``DINOTransformerDecoderLayer``,
    transformer.py:747-765; ``DeformableTransformerDecoderLayer`` in trees that keep DINO's own name) so that every layer built
    from then on has its ``nn.MultiheadAttention`` replaced by ``semi_detr_amd.MultiheadAttention``
    (``self_attn.convert_self_attention``: same parameters, same ``state_dict`` keys).  Returns (bound, skipped) names."""
    import functools
    import importlib

    from .self_attn import convert_self_attention
    layers = ("DINOTransformerDecoderLayer", "DeformableTransformerDecoderLayer")
    try:
        m = importlib.import_module("detr_od.models.utils.transformer")
    except ImportError:
        return [], [layers[0] + ".self_attn"]
    cls = next((getattr(m, n) for n in layers if hasattr(m, n)), None)
    if cls is None:
        return [], [layers[0] + ".self_attn"]
    names = [cls.__name__ + ".self_attn"]
    init = cls.__init__
    if not getattr(init, "_semidetr_self_attn", False):
        @functools.wraps(init)
        def wrapped(self, *args, **kwargs):
            init(self, *args, **kwargs)
            convert_self_attention(self)
        wrapped._semidetr_self_attn = True
        cls.__init__ = wrapped
    return names, []


def bind_layer_epilogues():
    """Where ``detr_od`` is importable, rebind the transformer layers to the fused residual add + LayerNorm + positional add of
    ``semi_detr_amd.add_norm``: ``DINOTransformerEncoderLayer.forward_ffn`` / ``.forward``, ``DINOTransformerEncoder.forward``
    (which threads ``output + pos`` from layer to layer) and ``DINOTransformerDecoderLayer.forward_ffn`` / ``.forward_sa`` /
    ``.forward_ca`` / ``.forward`` (``DeformableTransformer*Layer`` in trees that keep DINO's own layer names).  The layers' ``nn.LayerNorm``
    modules stay where they are: the epilogue reads their ``weight``, ``bias`` and ``eps``.  Idempotent.  Returns
    (bound, skipped) names."""
    import importlib

    from . import add_norm
    table = ((("DINOTransformerEncoderLayer", "DeformableTransformerEncoderLayer"),
              (("forward_ffn", add_norm.encoder_layer_forward_ffn), ("forward", add_norm.encoder_layer_forward))),
             (("DINOTransformerEncoder",), (("forward", add_norm.encoder_forward),)),
             (("DINOTransformerDecoderLayer", "DeformableTransformerDecoderLayer"),
              (("forward_ffn", add_norm.decoder_layer_forward_ffn), ("forward_sa", add_norm.decoder_layer_forward_sa),
               ("forward_ca", add_norm.decoder_layer_forward_ca), ("forward", add_norm.decoder_layer_forward))))
    try:
        m = importlib.import_module("detr_od.models.utils.transformer")
    except ImportError:
        m = None
    done, skipped = [], []
    for classes, methods in table:
        cls = next((getattr(m, n) for n in classes if hasattr(m, n)), None) if m is not None else None
        for name, fn in methods:
            if cls is None:
                skipped.append(f"{classes[0]}.{name}")
            else:
                setattr(cls, name, fn)              # a plain function: binds as a method, the layer is its first argument
                done.append(f"{cls.__name__}.{name}")
    return done, skipped
