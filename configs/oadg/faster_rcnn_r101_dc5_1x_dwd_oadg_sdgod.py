# OA-DG on the Diverse-Weather benchmark trained from its own files: the DWD OA-DG config with the reference's S-DGOD
# training set (configs/_base_/datasets/s-dgod.py:32-39 - RepeatDataset(times=2) over SdgodDataset on daytime-clear) and
# its complete train pipeline list (s-dgod.py:6-15) with the OA-Mix 'augmix.all' block (configs/OA-DG/_base_/dwd_oamix.py)
# ahead of Normalize.  Override data_root with --cfg-options data.train.dataset.{ann_file,img_prefix}=...; with the files
# absent, tools/train.py falls back to the synthetic source (with a notice).  The bench config
# (faster_rcnn_r101_dc5_1x_dwd_oadg.py) keeps its fixed 720x1280 synthetic batches.
_base_ = ['./faster_rcnn_r101_dc5_1x_dwd_oadg.py']
dataset_type = 'SdgodDataset'
data_root = 'data/S-DGOD/'
num_views = 2
img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
train_pipeline = [
    dict(type='LoadImageFromFile'),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='Resize', img_scale=[(1280, 600), (1280, 720)], keep_ratio=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='OAMix', version='augmix.all', num_views=num_views, keep_orig=True,
         use_mix=True, mixture_width=1, mixture_depth=-1, use_oa=True, oa_version='saliency_sparse',
         use_mrange=False, use_multilevel=True),
    dict(type='Normalize', **img_norm_cfg),
    dict(type='Pad', size_divisor=32),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'img2', 'gt_bboxes', 'gt_bboxes2', 'gt_labels', 'multilevel_boxes',
                               'oamix_boxes']),
]
data = dict(
    train=dict(
        _delete_=True,
        type='RepeatDataset',
        times=2,
        dataset=dict(
            type=dataset_type,
            ann_file=data_root + 'Daytime_Sunny/daytime_clear/VOC2007/ImageSets/Main/train.txt',
            img_prefix=data_root + 'Daytime_Sunny/daytime_clear/VOC2007/',
            pipeline=train_pipeline)))
