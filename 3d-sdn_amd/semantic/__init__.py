"""The semantic branch around the caller's network, on the device: the training batch (train_items: jitter, flip, resize,
labels), the pyramid pooling module inside the decoder (ppm: pool, upsample, concat around the caller's branch modules), the
training loss (train_loss: NLL of both decoder heads, deep supervision, pixel accuracy) and the tail (segm_tail: decoder scores to
label maps and to the evaluation's integers).  The segmentation network itself (semantic/models.py) is the caller's."""
from .ppm import ppm_bins, ppm_concat, ppm_fill, ppm_lerp, ppm_pool, use_device_ppm  # noqa: F401
from .segm_tail import SegmEvaluator, color_table, fuse_predictions, labels_from_colors, predict, summarize  # noqa: F401
from .train_items import batch_sizes, draw_item, jitter_params, label_formula, segm_train_batch, table_buffer  # noqa: F401
from .train_loss import segm_losses, train_forward  # noqa: F401
