# Augmentation baseline "photometric distortion": the baseline Faster R-CNN R50-FPN plus PhotoMetricDistortion (with its
# defaults: brightness_delta=32, contrast / saturation range (0.5, 1.5), hue_delta=18) in the train pipeline - one of the
# rows OA-DG is compared against on Cityscapes-C.  The step runs fused with Normalize and Pad (csrc/photo.hip).
_base_ = ['./faster_rcnn_r50_fpn_1x_cityscapes.py']
img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
train_pipeline = [
    dict(type='PhotoMetricDistortion'),
    dict(type='Normalize', **img_norm_cfg),
    dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]
data = dict(train=dict(pipeline=train_pipeline))
