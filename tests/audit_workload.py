"""The audited training steps shared by tests/test_conv_audit.py and tests/test_head_audit.py: the detector, optimizer and
device pipeline built as bench.py main() builds them, one unaudited step (its optimizer step refreshes the prepared-weight
bank), then a second step run under an auditor."""
import os
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R50_CFG = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r50_fpn_1x_cityscapes_oadg.py')
DC5_CFG = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r101_dc5_1x_dwd_oadg.py')


def audited_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size, install, on_begin=None,
                 on_end_backward=None, before_step1=None, speculative_sampling=None, amp_dtype=torch.bfloat16):
    """(out of the audited step, det, wall seconds).  ``install(monkeypatch, det)`` wraps the entry points after step 1;
    ``on_begin()`` / ``on_end_backward(det)`` run inside hip_conv.begin_step / end_backward of the audited step;
    ``before_step1(monkeypatch, det)`` may wrap something for step 1 as well (it stays installed for step 2);
    ``speculative_sampling`` (not None) sets TrainEngine.speculative_sampling - False: the RoI sampler draws on the host;
    ``amp_dtype`` None: the fp32 parity step of ``bench.py --dtype fp32`` (no hip_conv.enable(), fp32 pipeline, and
    begin_step(defer=False): the deferred path is bf16's)."""
    from oadg_amd import Config, build_detector, hip_conv
    from oadg_amd.apis import TrainEngine, build_optimizer, set_random_seed
    from oadg_amd.pipelines import DevicePipeline, SyntheticCityscapes
    cfg = Config.fromfile(cfg_path)
    if amp_dtype is not None:
        hip_conv.enable()
    try:
        set_random_seed(0)                       # bench.py main(): the same construction
        det = build_detector(cfg.model)
        det.init_weights(allow_missing_pretrained=True)
        det = det.to(dev).to(memory_format=torch.channels_last).train()
        det.log_vars_on_host = False
        engine = TrainEngine(det, build_optimizer(det, cfg.optimizer), amp_dtype=amp_dtype)
        if speculative_sampling is not None:
            engine.speculative_sampling = speculative_sampling
        set_random_seed(1)
        ds = SyntheticCityscapes(img_shape=(H, W), num_boxes=boxes, num_classes=classes, box_size=box_size, seed=0,
                                 device=dev)
        pipe = DevicePipeline(cfg.data.train.pipeline, dtype=amp_dtype or torch.float32)
        if before_step1 is not None:
            before_step1(monkeypatch, det)
        engine.step(pipe(*ds.batch(range(batch))))          # step 1: its optimizer step refreshes the prepared-weight bank
        data = pipe(*ds.batch(range(batch, 2 * batch)))
        torch.cuda.synchronize()

        install(monkeypatch, det)
        begin, end = hip_conv.begin_step, hip_conv.end_backward

        def begin_step(defer):
            if amp_dtype is torch.bfloat16:
                assert defer, 'the audited step must take the deferred path of TrainEngine._step'
            else:
                assert not defer, 'an fp32 step defers nothing'
            if on_begin is not None:
                on_begin()
            return begin(defer)

        def end_backward():
            n = end()
            torch.cuda.synchronize()
            if on_end_backward is not None:
                on_end_backward(det)
            return n
        monkeypatch.setattr(hip_conv, 'begin_step', begin_step)
        monkeypatch.setattr(hip_conv, 'end_backward', end_backward)
        t0 = time.perf_counter()
        out = engine.step(data)                             # step 2: audited
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        monkeypatch.undo()
        assert torch.isfinite(out['loss']).all()
        return out, det, wall
    finally:
        hip_conv.enable(False)


def tta_pipeline(img_scale, flip=False):
    """the reference's Cityscapes / DWD test pipeline (MultiScaleFlipAug over Resize(keep_ratio) ... Pad(32))"""
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
    inner = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **norm),
             dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]
    return [dict(type='LoadImageFromFile'), dict(type='MultiScaleFlipAug', img_scale=img_scale, flip=flip, transforms=inner)]


def audited_inference(dev, monkeypatch, tmp_path, cfg_path, batch, H, W, install, pipeline=None, on_forward=None):
    """(results of the two forwards, model, wall seconds of each) of bf16 test-time inference as tools/test.py runs it:
    build_model on a checkpoint file of deterministic weights (tests/golden/inputs.py named_weights), batches of the test
    pipeline (DevicePipeline.test_batch; ``pipeline`` overrides the config's), ``model(return_loss=False, rescale=True)``
    under no_grad and bf16 autocast.  ``install(monkeypatch, model)`` wraps the entry points before the first forward (cold:
    the weight preparation launches) and stays installed for the second (served from the bank); ``on_forward(k, model,
    results, data)`` runs after forward k (0, 1) with the batch it ran on."""
    from inputs import named_weights
    from oadg_amd import Config, build_detector, hip_conv
    from oadg_amd.apis import set_random_seed
    from oadg_amd.pipelines import DevicePipeline, SyntheticCityscapes
    from test_cli import _load
    test_tool = _load('test')
    cfg = Config.fromfile(cfg_path)
    ck = str(tmp_path / 'weights.pth')
    try:
        set_random_seed(0)
        shapes = {k: v.shape for k, v in build_detector(Config.fromfile(cfg_path).model).state_dict().items()}
        torch.save({'state_dict': {k: torch.as_tensor(v) for k, v in named_weights(shapes).items()}}, ck)
        model = test_tool.build_model(cfg, ck, dev, torch.bfloat16)
        assert hip_conv.ENABLED and not model.training
        pipe = DevicePipeline(pipeline if pipeline is not None else cfg.data.test.pipeline, dtype=torch.bfloat16)
        ds = SyntheticCityscapes(img_shape=(H, W), num_boxes=12, box_size=(24, 300), seed=3, device=dev)
        imgs, _, _ = ds.batch(list(range(batch)))
        install(monkeypatch, model)
        outs, walls = [], []
        for k in range(2):
            data = pipe.test_batch(imgs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                res = model(return_loss=False, rescale=True, **data)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
            outs.append(res)
            if on_forward is not None:
                on_forward(k, model, res, data)
        monkeypatch.undo()
        return outs, model, walls
    finally:
        hip_conv.enable(False)
