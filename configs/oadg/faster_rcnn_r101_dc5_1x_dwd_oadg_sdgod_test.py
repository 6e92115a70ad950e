# The S-DGOD config with the reference's evaluation side: its test pipeline (configs/_base_/datasets/s-dgod.py:16-30), the
# daytime-clear validation split (s-dgod.py:42-46), the five Diverse-Weather test splits as the list tools/test_dwd.py walks
# (s-dgod.py:82-108: daytime-clear test.txt, then foggy / dusk-rainy / night-rainy / night-sunny train.txt, each with a
# one-entry ann_file / img_prefix list -> a ConcatDataset of one SdgodDataset) and the VOC07 mAP after every epoch
# (s-dgod.py:111).  Training is the inherited config's.  Override data_root with --cfg-options data.test.N.ann_file=... .
_base_ = ['./faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod.py']
dataset_type = 'SdgodDataset'
data_root = 'data/S-DGOD/'
img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
test_pipeline = [
    dict(type='LoadImageFromFile'),
    dict(
        type='MultiScaleFlipAug',
        img_scale=(2048, 1024),
        flip=False,
        transforms=[
            dict(type='Resize', keep_ratio=True),
            dict(type='RandomFlip'),
            dict(type='Normalize', **img_norm_cfg),
            dict(type='Pad', size_divisor=32),
            dict(type='ImageToTensor', keys=['img']),
            dict(type='Collect', keys=['img']),
        ])
]
data = dict(
    val=dict(
        type=dataset_type,
        ann_file=data_root + 'Daytime_Sunny/daytime_clear/VOC2007/ImageSets/Main/test.txt',
        img_prefix=data_root + 'Daytime_Sunny/daytime_clear/VOC2007/',
        pipeline=test_pipeline),
    test=[
        dict(
            type=dataset_type,
            ann_file=[data_root + 'Daytime_Sunny/daytime_clear/VOC2007/ImageSets/Main/test.txt'],
            img_prefix=[data_root + 'Daytime_Sunny/daytime_clear/VOC2007/'],
            pipeline=test_pipeline),
        dict(
            type=dataset_type,
            ann_file=[data_root + 'Daytime-Foggy/daytime_foggy/VOC2007/ImageSets/Main/train.txt'],
            img_prefix=[data_root + 'Daytime-Foggy/daytime_foggy/VOC2007/'],
            pipeline=test_pipeline),
        dict(
            type=dataset_type,
            ann_file=[data_root + 'Dusk-rainy/dusk_rainy/VOC2007/ImageSets/Main/train.txt'],
            img_prefix=[data_root + 'Dusk-rainy/dusk_rainy/VOC2007/'],
            pipeline=test_pipeline),
        dict(
            type=dataset_type,
            ann_file=[data_root + 'Night_rainy/night_rainy/VOC2007/ImageSets/Main/train.txt'],
            img_prefix=[data_root + 'Night_rainy/night_rainy/VOC2007/'],
            pipeline=test_pipeline),
        dict(
            type=dataset_type,
            ann_file=[data_root + 'Night-Sunny/night_sunny/VOC2007/ImageSets/Main/train.txt'],
            img_prefix=[data_root + 'Night-Sunny/night_sunny/VOC2007/'],
            pipeline=test_pipeline),
    ])
evaluation = dict(interval=1, metric='mAP')
