# The first stage of the Cityscapes Faster R-CNN R50-FPN on its own: backbone, neck and RPN head of
# ../oadg/faster_rcnn_r50_fpn_1x_cityscapes.py as an 'RPN' detector, whose test returns the proposals of every image.  A
# checkpoint trained with that config (or with its OA-DG variant) loads into it; its roi_head.* tensors are unexpected, nothing
# else.  tools/test.py CONFIG CKPT --eval proposal_fast reports AR@100 / 300 / 1000 of those proposals.
# roi_head=None: inheritance cannot remove a key, the detector takes None for "no second stage".
# test_cfg.rpn holds the FASTER R-CNN's own test values (_base_/faster_rcnn_r50_fpn.py: nms_pre 1000, max_per_img 1000, NMS
# at 0.7), not the 2000 / 1000 of an RPN trained alone: these are the proposals its second stage really sees.
_base_ = ['../oadg/faster_rcnn_r50_fpn_1x_cityscapes.py']
model = dict(type='RPN', roi_head=None,
             test_cfg=dict(_delete_=True,
                           rpn=dict(nms_pre=1000, max_per_img=1000, nms=dict(type='nms', iou_threshold=0.7),
                                    min_bbox_size=0)))
# No `evaluation` key of its own: the proposal metrics are asked for on the command line (tools/test.py --eval ...); EvalHook
# and dataset.evaluate do not take them yet (oadg_recall.py's docstring has the follow-up), and an RPN is not trained here.
