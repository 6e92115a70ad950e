# Augmentation baseline "Cutout": the baseline Faster R-CNN R50-FPN plus CutOut in the train pipeline - one of the rows OA-DG
# is compared against on Cityscapes-C.  The number of holes and the candidate ratios (fractions of the image's width and
# height) are THIS project's choice, not the paper's, which does not state them.  The step runs fused with Normalize and Pad
# (csrc/photo.hip).
_base_ = ['./faster_rcnn_r50_fpn_1x_cityscapes.py']
img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
train_pipeline = [
    dict(type='CutOut', n_holes=(1, 5), cutout_ratio=[(0.05, 0.1), (0.1, 0.2), (0.15, 0.3)], fill_in=(0, 0, 0)),
    dict(type='Normalize', **img_norm_cfg),
    dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]
data = dict(train=dict(pipeline=train_pipeline))
