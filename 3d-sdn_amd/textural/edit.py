"""Editing a scene: what the reference's textural/edit_vkitti.py and edit_benchmark.py do around the model.

The source frame is encoded ONCE into one appearance code per instance (`netE.generate_feat_dict`, edit_vkitti.py:57).  For
every edited frame the geometric branch wrote (NNNNN.png + NNNNN.json + NNNNN-normal.png) the label, instance, pose and
normal inputs are rebuilt (:63-95), each instance's SOURCE code is painted at the instance's NEW pixels (:97-103) and the
generator runs on them (`fake_inference(..., feat=...)`, :105).  The code follows the object: a moved or rotated car keeps
its colour.

Here the code table stays on the device (`Encoder.feat_table`), the assembly of F edited frames is one kernel launch
(`data.assemble.assemble_edit` -> sdn_edit_assemble) and the F frames go through the generator as one batch.  The only
device-to-host copy of a call is the read-back of the per-frame count of pixels whose instance has no source code.
"""
import torch

from data import assemble as _asm


class EditSession:
    """One source frame, any number of edited frames.

    model          a Pix2PixHDModel with an encoder (instance_feat, not load_features)
    opt, params    the options / get_params dict the loader would use (data.assemble.assemble_item)
    base_segm_u8   uint8 [1, H, W]  the source frame's label map (opt.segm_precomputed_path)
    base_image_u8  uint8 [3, H, W]  the source frame
    base_inst_u8   uint8 [1, H, W]  the source frame's raw object ids (NNNNN.png of the unedited scene, "00000.png")
    All three on the GPU.  `session.codes` = (ids, means [K, feat_num]) and `session.counts` [K] describe the source."""

    def __init__(self, model, opt, params, base_segm_u8, base_image_u8, base_inst_u8):
        for t, name in ((base_segm_u8, 'base_segm_u8'), (base_image_u8, 'base_image_u8'), (base_inst_u8, 'base_inst_u8')):
            if not isinstance(t, torch.Tensor):
                raise TypeError('%s must be a torch.Tensor' % name)
            if not t.is_cuda:
                raise NotImplementedError('%s is on %s; an edit session only runs on the GPU' % (name, t.device))
        if not (opt.segm_precomputed_path and opt.inst_precomputed_path):
            raise ValueError('an edit needs segm_precomputed_path and inst_precomputed_path (edit_vkitti.py:42-54)')
        if not getattr(model, 'gen_features', False):
            raise ValueError('the model has no feature encoder (instance_feat without load_features)')
        self.model, self.opt, self.params = model, opt, params
        self.base_item = _asm.assemble_item(opt, params, base_segm_u8, base_image_u8, inst=base_inst_u8)
        with torch.no_grad():
            ids, means, counts = model.netE.feat_table(self.base_item['image'][None], self.base_item['inst'][None].clone())
        self.codes, self.counts = (ids, means), counts
        self.last_missing = None
        self.last_inputs = None

    def render(self, edit_inst_u8, edit_json, normal_u8=None, strict=True):
        """The generated image [1, 3, h, w] of one edited frame."""
        return self.render_batch([(edit_inst_u8, edit_json, normal_u8)], strict=strict)

    def render_batch(self, frames, strict=True):
        """frames: a list of (edit_inst_u8, edit_json, normal_u8 or None).  One assembly launch and one fake_inference
        for all of them; returns [F, 3, h, w].  strict: an instance of an edited frame without a source code raises
        KeyError naming the frame (edit_vkitti.py:103 would); otherwise its pixels are painted 0 (edit_benchmark.py:121-123)
        and `last_missing` lists the pixel count per frame."""
        frames = [tuple(fr) + (None,) * (3 - len(fr)) for fr in frames]
        x = _asm.assemble_edit(self.opt, self.params, self.base_item, [fr[0] for fr in frames], [fr[1] for fr in frames],
                               self.codes, [fr[2] for fr in frames])
        self.last_inputs = x
        self.last_missing = x['missing'].cpu().tolist()   # the call's one device-to-host copy
        if strict and any(self.last_missing):
            bad = [k for k, n in enumerate(self.last_missing) if n]
            raise KeyError('edited frame(s) %s: %s pixels belong to instances the source frame has no code for'
                           % (bad, [self.last_missing[k] for k in bad]))
        F = len(frames)
        image = self.base_item['image'][None].expand(F, -1, -1, -1)
        return self.model.fake_inference(image, x['label'], x['inst'], feat=x['feat'], pose=x['pose'], normal=x['normal'])
