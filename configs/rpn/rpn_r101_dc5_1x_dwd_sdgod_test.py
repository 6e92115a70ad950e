# The first stage of the Diverse-Weather Faster R-CNN R101-DC5 on its own, over the five S-DGOD test splits of
# ../oadg/faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod_test.py (data.test is that config's list: daytime-clear, foggy, dusk-rainy,
# night-rainy, night-sunny).  A checkpoint trained with the OA-DG DWD config loads into it; its roi_head.* tensors are
# unexpected, nothing else.  tools/test.py CONFIG CKPT --eval recall reports recall@100 / 300 / 1000 per split: which
# domains lose their objects already in the first stage.
# roi_head=None: inheritance cannot remove a key, the detector takes None for "no second stage".
# test_cfg.rpn holds the FASTER R-CNN's own test values (_base_/faster_rcnn_r50_caffe_dc5.py: nms_pre 6000, max_per_img 1000,
# NMS at 0.7): these are the proposals its second stage really sees.
_base_ = ['../oadg/faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod_test.py']
model = dict(type='RPN', neck=None, roi_head=None,          # (a dilated C5 backbone: no neck)
             test_cfg=dict(_delete_=True,
                           rpn=dict(nms=dict(type='nms', iou_threshold=0.7), nms_pre=6000, max_per_img=1000,
                                    min_bbox_size=0)))
# No `evaluation` key of its own (the inherited one names 'mAP', a detection metric): the proposal metrics are asked for on the
# command line (tools/test.py --eval recall); EvalHook and dataset.evaluate do not take them yet (oadg_recall.py's docstring
# has the follow-up), and an RPN is not trained here.
