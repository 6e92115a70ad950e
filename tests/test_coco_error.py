"""CPU: the COCO error analysis on the host.  ``evaluation.coco_error_flags_host`` (the yardstick of csrc/coco_error.hip) on
hand cases whose flags are written out; ``coco_error_analysis(device=None)`` against the reference tool's algorithm done the
long way on a seeded split; the COCO result file (``format_results``, ``tools/test.py --format-only``, ``eval_metric.py
--format-only``) and its round trip through the loader of tools/analysis_tools/coco_error_analysis.py; the tool itself with
``--device host``.  Every comparison is == on integers or np.array_equal on fp64."""
import json
import os

import numpy as np
import pytest

import coco_error_cases as C
from oadg_amd import evaluation as E

TOOL = 'tools/analysis_tools/coco_error_analysis.py'


# ------------------------------------------------------------------------------------------------------------ hand cases
@pytest.mark.parametrize('name', sorted(C.hand_cases()))
def test_hand_case_flags(name):
    images, K, sup, want = C.hand_cases()[name]
    flags = E.coco_error_flags_host(C.pack_images(images, K, sup), C.THRS, C.SIM, C.AREA_RNG)
    assert flags.shape[:2] == (4, 5) and flags.dtype == np.uint8
    for a, rows in want.items():
        assert flags[a].T.tolist() == rows, (name, a)


def test_pack_holds_every_box_of_an_image_once():
    gt_anns, results = C.seeded_split()
    pack = E.pack_coco_error(gt_anns, results, 6, C.SUPERCATS)
    plain = E.pack_coco_segments(gt_anns, results, 6, 100)
    assert len(pack['gts']) == sum(len(g) for g in gt_anns) == len(plain['gts'])
    assert np.diff(pack['img_off']).tolist() == [len(g) for g in gt_anns] and pack['img_off'].dtype == np.int32
    assert pack['cat_super'].tolist() == C.SUPERCATS and pack['gt_cat'].dtype == np.int32
    for k in ('dets', 'det_off', 'det_score', 'det_rank', 'det_cat'):
        assert np.array_equal(pack[k], plain[k]), k
    assert E.pack_coco_error(gt_anns, results, 6, list('aaabbc'))['cat_super'].tolist() == C.SUPERCATS
    # the plain rows are the plain evaluation's flags
    flags = E.coco_error_flags_host(pack, C.THRS, C.SIM, C.AREA_RNG)
    assert np.array_equal(flags[:, :3], E.coco_flags_host(plain, C.THRS, C.AREA_RNG, iou_thrs=C.THRS))


# ------------------------------------------------------------------------------------------------------------ seeded split
@pytest.fixture(scope='module')
def split():
    return C.seeded_split()


@pytest.fixture(scope='module')
def ps(split):
    return E.coco_error_analysis(*split, 6, C.SUPERCATS, areas=C.AREAS, device=None)


def test_seeded_split_is_what_the_suite_says(split):
    gt_anns, results = split
    assert len(gt_anns) == 12 and not gt_anns[3] and sum(len(r) for r in results[5]) == 0
    assert all(len(per) == 6 for per in results) and any(g['iscrowd'] for per in gt_anns for g in per)
    scores = np.concatenate([r[:, 4] for per in results for r in per])
    assert len(np.unique(scores)) <= 11 < len(scores)                    # ties


def test_analysis_equals_the_tool_done_the_long_way(split, ps):
    want = C.long_way(*split, 6, C.SUPERCATS)
    assert ps.shape == want.shape == (7, 101, 6, 4, 1) and ps.dtype == np.float64
    assert np.array_equal(ps, want)


def test_bands_are_strictly_increasing_and_a_lone_class_has_sim_equal_loc(ps):
    """all classes, all areas, with this generator: 0.0233 < 0.0320 < 0.0663 < 0.0791 < 0.1602 < 0.4026 < 1 - a variant row that
    silently repeated another could not pass; class 5 is alone in its supercategory, classes 0 - 4 are not.  (The distributions
    are the ones the suite was specified with; a first prototype of it drew its random numbers in another order and gave 0.0090
    < 0.0241 < 0.0538 < 0.0645 < 0.1317 < 0.3218 < 1: other boxes, the same ordering.)"""
    means = [float(ps[b][..., 0, 0].mean()) for b in range(7)]
    assert all(a < b for a, b in zip(means, means[1:])) and means[6] == 1.0
    assert np.array_equal(ps[3][:, 5], ps[2][:, 5])
    assert not any(np.array_equal(ps[3][:, k], ps[2][:, k]) for k in range(5))
    assert set(np.unique(ps[5]).tolist()) == {0.0, 1.0}
    m = E.error_band_means(ps, C.NAMES)
    assert list(m) == list(C.NAMES) + ['allclass'] and m['allclass']['allarea']['Oth'] == means[4]
    assert m['train']['small']['Sim'] == float(ps[3][:, 5, 1, 0].mean())


def test_default_arguments_of_the_evaluator_are_unchanged(split):
    gt_anns, results = split
    pack = E.pack_coco_segments(gt_anns, results, 6, 100)
    flags = E.coco_flags_host(pack)
    assert np.array_equal(flags, E.coco_flags_host(pack, E.IOU_THRS, E.AREA_RNG, iou_thrs=E.IOU_THRS))
    a, b = E.coco_accumulate(pack, flags, [1, 10, 100]), E.coco_accumulate(pack, flags, [1, 10, 100], E.IOU_THRS, E.AREA_RNG)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert E.coco_summarize(*a) == E.coco_eval_bbox(gt_anns, results, 6)
    with pytest.raises(ValueError, match='IOU_THRS only'):
        E.coco_flags_host(pack, [0.1])


# ------------------------------------------------------------------------------------------------------------ result file
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """a small split as files: 6 images, 3 classes (person, rider | car), ids that are not 0 .. n"""
    d = tmp_path_factory.mktemp('coco_error')
    gt_anns, results = C.seeded_split(3, n_img=6, n_cls=3)
    names = C.NAMES[:3]
    ann = C.write_ann(d / 'ann.json', gt_anns, names, supercategory=['human', 'human', 'vehicle'])
    bare = C.write_ann(d / 'bare.json', gt_anns, names)
    ds = C.coco_dataset(ann, names)
    out, tmp = ds.format_results(results, jsonfile_prefix=str(d / 'res' / 'dets'))
    assert tmp is None and out == dict(bbox=str(d / 'res' / 'dets.bbox.json'), proposal=str(d / 'res' / 'dets.bbox.json'))
    return dict(dir=d, gt_anns=gt_anns, results=results, names=names, ann=ann, bare=bare, ds=ds, res=out['bbox'])


def test_format_results_round_trip(files):
    ds, results = files['ds'], files['results']
    assert ds.cat_ids == [3, 5, 7] and ds.img_ids[:3] == [10, 13, 16]
    records = json.load(open(files['res']))
    assert len(records) == sum(len(r) for per in results for r in per) > 50
    first = next(r for r in results[0] if len(r))[0]
    assert set(records[0]) == {'image_id', 'bbox', 'score', 'category_id'} and records[0]['image_id'] == 10
    assert records[0]['bbox'] == [float(first[0]), float(first[1]), float(first[2]) - float(first[0]), float(first[3]) - float(first[1])]
    assert {r['category_id'] for r in records} == {3, 5, 7} and {r['image_id'] for r in records} <= set(ds.img_ids)
    T = C.load_tool(TOOL)
    cats, gt_anns, back, areas = T.load_split(files['ann'], files['res'])
    assert [c['name'] for c in cats] == list(files['names']) and gt_anns == files['gt_anns'] and len(areas) == sum(map(len, gt_anns))
    for per, per_back in zip(results, back):
        for r, b in zip(per, per_back):
            r = r.astype(np.float64)
            want = np.stack([r[:, 0], r[:, 1], r[:, 2] - r[:, 0], r[:, 3] - r[:, 1], r[:, 4]], 1)
            assert b.dtype == np.float64 and np.array_equal(b, want)
    # so the file evaluates to what the arrays evaluate to
    sup = ['human', 'human', 'vehicle']
    assert np.array_equal(E.coco_error_analysis(gt_anns, back, 3, sup, xywh=True),
                          E.coco_error_analysis(files['gt_anns'], results, 3, sup))
    # without a prefix: a temporary directory that the caller owns
    out, tmp = ds.format_results(results)
    assert os.path.dirname(out['bbox']) == tmp.name and json.load(open(out['bbox'])) == records
    tmp.cleanup()
    with pytest.raises(AssertionError, match='length of results'):
        ds.format_results(results[:-1])
    with pytest.raises(TypeError, match='invalid type of results'):
        ds.format_results([np.zeros((0, 5))] * len(ds))
    with pytest.raises(NotImplementedError, match="'jsonfile_prefix'"):       # evaluate() still has no such keyword
        ds.evaluate(results, metric='bbox', jsonfile_prefix='x')


def test_test_tool_format_only_writes_the_file_without_evaluating(files, capsys, monkeypatch):
    monkeypatch.setenv('LOCAL_RANK', '0')                                     # (parse_args sets a default for it)
    T = C.load_tool('tools/test.py')
    monkeypatch.setattr('sys.argv', ['test.py', 'cfg.py', 'none', '--format-only', '--eval-options', 'jsonfile_prefix=x/y'])
    a = T.parse_args()
    assert a.format_only and a.eval_options == dict(jsonfile_prefix='x/y') and not a.eval
    monkeypatch.setattr('sys.argv', ['test.py', 'cfg.py', 'none', '--format-only', '--eval', 'bbox'])
    with pytest.raises(ValueError, match='cannot be both specified'):
        T.parse_args()
    with pytest.raises(NotImplementedError, match='--format-only: cfg.data.test is a list of 5 splits'):
        T.check_splits_arguments(a, 5)
    # what main() does once the split is tested: with --format-only the file is written and nothing is evaluated ...
    calls = []
    monkeypatch.setattr(T, 'evaluate', lambda *args, **kw: calls.append(args) or dict(bbox=dict(mAP=0.0)))
    prefix = str(files['dir'] / 'from_test_tool' / 'r')
    a.eval_options = dict(jsonfile_prefix=prefix)
    out = T.report(a, files['results'][:4], files['ds'], dict(num_classes=3))                # (--max-samples 4)
    assert out['bbox'] == prefix + '.bbox.json' and 'writing results to' in capsys.readouterr().out and not calls
    # ... and the same call with --eval instead does evaluate (the guard above can fire)
    monkeypatch.setattr('sys.argv', ['test.py', 'cfg.py', 'none', '--eval', 'bbox'])
    T.report(T.parse_args(), files['results'], files['ds'], dict(num_classes=3))
    assert len(calls) == 1 and 'bbox (COCO style)' in capsys.readouterr().out
    want = [r for r in json.load(open(files['res'])) if r['image_id'] in files['ds'].img_ids[:4]]
    assert json.load(open(out['bbox'])) == want
    none = T.format_only(files['ds'], files['results'], None)
    assert not os.path.exists(none['bbox']) and 'temporary directory' in capsys.readouterr().out


def test_eval_metric_format_only_calls_format_results(files, tmp_path, capsys):
    import pickle
    M = C.load_tool('tools/analysis_tools/eval_metric.py')
    cfg, pkl = tmp_path / 'cfg.py', tmp_path / 'r.pkl'
    cfg.write_text(f"data = dict(test=dict(type='CocoDataset', ann_file={files['ann']!r}, classes={tuple(files['names'])!r}, "
                   f"img_prefix='', pipeline=[]))\n")
    with open(pkl, 'wb') as f:
        pickle.dump(files['results'], f)
    out = M.main([str(cfg), str(pkl), '--format-only', '--eval-options', f'jsonfile_prefix={tmp_path / "m"}'])
    assert out['bbox'] == str(tmp_path / 'm.bbox.json') and open(out['bbox']).read() == open(files['res']).read()
    with pytest.raises(ValueError, match='cannot be both specified'):
        M.parse_args([str(cfg), str(pkl), '--format-only', '--eval', 'bbox'])
    with pytest.raises(SystemExit):
        M.parse_args([str(cfg), str(pkl)])


# ------------------------------------------------------------------------------------------------------------ the tool
def test_tool_on_the_host(files, tmp_path, capsys):
    from PIL import Image
    T = C.load_tool(TOOL)
    out = tmp_path / 'out'
    got = T.main([files['res'], str(out), '--ann', files['ann'], '--device', 'host', '--extraplots'])
    sup = ['human', 'human', 'vehicle']
    ps = E.coco_error_analysis(files['gt_anns'], files['results'], 3, sup)
    assert np.array_equal(got['bbox'], ps)
    stems = [f'bbox-{c}-{a}' for c in list(files['names']) + ['allclass'] for a in E.ERROR_AREA_NAMES]
    stems += [f'bbox-{c}-ap bar plot' for c in list(files['names']) + ['allclass']]
    stems += ['number of annotations per area group', 'gt annotation areas histogram plot']
    assert sorted(os.listdir(out / 'bbox')) == sorted([s + '.png' for s in stems] + ['error_analysis.json'])
    with Image.open(out / 'bbox' / 'bbox-allclass-allarea.png') as im:
        im.load()
        assert im.format == 'PNG' and im.size[0] > 100 and im.size[1] > 100
    js = json.load(open(out / 'bbox' / 'error_analysis.json'))
    assert js['means'] == E.error_band_means(ps, files['names']) and js['types'] == list(E.ERROR_TYPES)
    assert js['classes'] == list(files['names']) and js['supercategories'] == sup and js['areas'] == [1024, 9216, 10 ** 10]
    counts = T.gt_area_group_numbers(files['gt_anns'], 3, E.error_area_rng(C.AREAS))
    assert counts['all'] == counts['small'] + counts['medium'] + counts['large'] > 0
    assert 'number of annotations per area group' in capsys.readouterr().out


def test_tool_supercategory_fallbacks_and_rejections(files, tmp_path, capsys):
    T = C.load_tool(TOOL)
    cats = json.load(open(files['bare']))['categories']
    assert all('supercategory' not in c for c in cats)
    assert T.supercategories(cats, ['cityscapes'], log=print) == ['human', 'human', 'vehicle']
    assert T.supercategories(cats, ['person=a', 'rider=b', 'car=b']) == ['a', 'b', 'b']
    own = T.supercategories(cats, None, log=print)
    assert len(set(own)) == 3 and 'Sim equals Loc' in capsys.readouterr().out
    assert own == ['person', 'rider', 'car']
    with_field = json.load(open(files['ann']))['categories']
    assert T.supercategories(with_field, None) == ['human', 'human', 'vehicle']
    with pytest.raises(ValueError, match='the annotation file names a supercategory'):       # the field is what is used
        T.supercategories(with_field, ['person=a', 'rider=b', 'car=b'])
    with pytest.raises(ValueError, match='names no supercategory'):
        T.supercategories(cats, ['person=a'])
    with pytest.raises(ValueError, match='name=super'):
        T.supercategories(cats, ['cityscapes', 'coco'])
    # the file without the field and no option: Sim is Loc
    with_field = T.analyze_results(files['res'], files['ann'], [], str(tmp_path / 'a'), device='host')
    assert with_field == {}
    ps = E.coco_error_analysis(files['gt_anns'], files['results'], 3, ['human', 'human', 'vehicle'])
    b = T.main([files['res'], str(tmp_path / 'c'), '--ann', files['bare'], '--device', 'host', '--areas', '900', '8000', '100000'])
    assert np.array_equal(b['bbox'][3], b['bbox'][2]) and not np.array_equal(ps[3], ps[2])
    assert not np.array_equal(b['bbox'][:3], ps[:3])                              # (--areas reached the evaluation)
    with pytest.raises(NotImplementedError, match='--types segm'):
        T.parse_args(['r.json', 'out', '--types', 'segm'])
    with pytest.raises(ValueError, match='3 integers'):
        T.parse_args(['r.json', 'out', '--areas', '1', '2'])
