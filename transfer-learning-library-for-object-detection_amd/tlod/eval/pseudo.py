"""Pseudo labels for IDF's target branch (step 3 of methods/IDF/IDF_train.sh): a source-only
detector labels the target images, and the ``_t`` detector trains on those boxes.

Two routes, held equal by tests/test_selftrain_{cpu,gpu}.py:

  * online — ``label_image``: the labeler's eval-mode forward under no_grad, tlod_detect_f32 with
    ``score_thresh = thresh`` (0.5 is the reference's --savelabel value, applied before the NMS
    as in faster_rcnn_test.py:318-333) and tlod_pseudo_gt_f32 (``pseudo_gt``), which packs the
    kept rows into the (1, max_gt, 5) gt_boxes / (1,) int64 num_boxes the models' forward takes.
    Three launches behind the labeler's own, nothing read back: the image scale and size come
    as host numbers.
  * offline — ``save_labels``: the reference's route.  Per image ``detect()``, the rows to the
    host, ``str(int(x))`` and the class name into ``Annotations/<index>.xml``
    (faster_rcnn_test.py:351-369, lib/IDF/xml_create.py); ``tlod.data.imdb.pseudo_voc`` reads
    them back with the IDF loaders' clamp and the training loader does the rest.

The packer's rule is the offline route applied to one image that needs no crop; where the loader
shuffles and keeps the first MAX_NUM_GT_BOXES, the packer keeps a uniform random subset chosen by
the device generator (stream ``PSEUDO_STREAM``) in the rows' original order.
"""
import os

import torch
from PIL import Image

from .. import _lib
from ..config import cfg
from .detect import ctypes_floats, detect

PSEUDO_STREAM = 0x70736575  # csrc/selftrain.hip
_M64 = (1 << 64) - 1


def pseudo_gt(dets, counts, im_scale, max_gt=None, seed=0):
    """dets (C, R, 5), counts (C,) int32 as ``detect`` leaves them, im_scale a host float (the
    loader's Python float, taken as a double) -> (gt_boxes (1, max_gt, 5) float32, num_boxes
    (1,) int64) on the device: tlod_pseudo_gt_f32, one launch.  max_gt: cfg.MAX_NUM_GT_BOXES."""
    _lib.require_cuda(dets, counts)
    dets = dets.detach().contiguous().float()
    assert dets.dim() == 3 and dets.shape[2] == 5, dets.shape
    C, R = dets.shape[:2]
    assert counts.dtype == torch.int32 and counts.numel() == C, (counts.dtype, counts.shape)
    counts = counts.contiguous()
    max_gt = int(cfg.MAX_NUM_GT_BOXES if max_gt is None else max_gt)
    # refused before anything is allocated (the entry point refuses them too)
    if max_gt < 1 or not float(im_scale) > 0.0:
        raise ValueError(f"pseudo_gt: max_gt {max_gt}, im_scale {im_scale}")
    gt = torch.empty((1, max_gt, 5), dtype=torch.float32, device=dets.device)
    num = torch.empty(1, dtype=torch.int64, device=dets.device)
    _lib.check(_lib.lib().tlod_pseudo_gt_f32(
        _lib.ptr(dets), _lib.ptr(counts), C, R, float(im_scale), max_gt, int(seed) & _M64,
        _lib.ptr(gt), _lib.ptr(num), _lib.stream_of(dets)), "pseudo_gt")
    return gt, num


def detect_host_info(rois, cls_prob, bbox_pred, im_h, im_w, im_scale, class_agnostic=False,
                     thresh=0.0, nms=None):
    """``tlod.eval.detect.detect`` with the image size and scale as host floats, so nothing is
    read back: (dets (C, R, 5), counts (C,) int32) on the device."""
    _lib.require_cuda(rois, cls_prob, bbox_pred)
    rois = rois.detach().reshape(-1, 5).contiguous().float()
    cls_prob = cls_prob.detach().reshape(rois.shape[0], -1).contiguous().float()
    R, C = cls_prob.shape
    bbox_pred = bbox_pred.detach().reshape(R, -1).contiguous().float()
    assert bbox_pred.shape[1] == (4 if class_agnostic else 4 * C), bbox_pred.shape
    pre = cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED
    stds = ctypes_floats(cfg.TRAIN.BBOX_NORMALIZE_STDS if pre else (1, 1, 1, 1))
    means = ctypes_floats(cfg.TRAIN.BBOX_NORMALIZE_MEANS if pre else (0, 0, 0, 0))
    dets = torch.empty((C, R, 5), dtype=torch.float32, device=rois.device)
    counts = torch.empty(C, dtype=torch.int32, device=rois.device)
    _lib.check(_lib.lib().tlod_detect_f32(
        _lib.ptr(rois), _lib.ptr(cls_prob), _lib.ptr(bbox_pred), R, C, int(class_agnostic), stds,
        means, float(im_h), float(im_w), float(im_scale), float(thresh),
        float(cfg.TEST.NMS if nms is None else nms), _lib.ptr(dets), _lib.ptr(counts), None,
        _lib.stream_of(rois)), "detect")
    return dets, counts


_consts = {}


def _labeler_inputs(device, info):
    """The device im_info of the host triple and the placeholder gt_boxes / num_boxes of an
    eval-mode forward, made once per (device, triple): later calls copy nothing."""
    key = (str(device), info)
    c = _consts.get(key)
    if c is None:
        c = _consts[key] = (torch.tensor([info], dtype=torch.float32, device=device),
                            torch.ones((1, 1, 5), dtype=torch.float32, device=device),
                            torch.zeros(1, dtype=torch.int64, device=device))
    return c


@torch.no_grad()
def label_image(labeler, data, im_info_host, thresh=0.5, class_agnostic=False, max_gt=None,
                seed=0):
    """Pseudo ground truth of one image (batch of 1) on the device, no host round trip.

    labeler: any eval-mode detector of this package (``build_model("faster_rcnn", ...).eval()``;
    its 4-argument forward gives rois, cls_prob, bbox_pred); data (1, 3, H, W);
    im_info_host = (height, width, scale) of the blob as host numbers, scale being the loader's
    Python float.  Returns (gt_boxes (1, max_gt, 5), num_boxes (1,) int64) in the blob's
    coordinates, as the training loader would hand them over."""
    if labeler.training:
        raise RuntimeError("label_image: put the labeler in eval mode (labeler.eval())")
    h, w, s = (float(v) for v in im_info_host)
    im_info, gt, num = _labeler_inputs(data.device, (h, w, s))
    rois, cls_prob, bbox_pred = labeler(data, im_info, gt, num)[:3]
    dets, counts = detect_host_info(rois[0], cls_prob[0], bbox_pred[0], h, w, s, class_agnostic,
                                    thresh)
    return pseudo_gt(dets, counts, s, max_gt, seed)


def label_objects(dets, counts, classes):
    """The XML objects of one image from host (C, R, 5) / (C,) arrays: class-major, each class
    in its kept order, coordinates truncated by the writer's ``str(int(x))``
    (faster_rcnn_test.py:357-361)."""
    return [(classes[j], *(float(v) for v in dets[j, i, :4]), 0)
            for j in range(1, dets.shape[0]) for i in range(int(counts[j]))]


def write_label_xml(devkit_out, year, index, height, width, objects):
    """``Annotations/<index>.xml`` with the standard VOC tags (tlod.data.synthetic's writer)."""
    from ..data.synthetic import _xml
    d = os.path.join(devkit_out, "VOC" + year, "Annotations")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, index + ".xml")
    _xml(index, height, width, objects).write(path)
    return path


@torch.no_grad()
def save_labels(labeler, imdb, loader, devkit_out, thresh=0.5, class_agnostic=False,
                image_set=None):
    """The offline route over a test roibatchLoader (training=False) of ``imdb``: one
    ``Annotations/<index>.xml`` per image under ``<devkit_out>/VOC<year>`` and the image-set
    file listing them.  No image is copied: read the result with
    ``pseudo_voc(image_set, year, devkit_out, classes, image_devkit=<imdb's devkit>)`` (or write
    into the images' own devkit).  Returns the number of boxes written per image."""
    if labeler.training:
        raise RuntimeError("save_labels: put the labeler in eval mode (labeler.eval())")
    year = imdb._year
    image_set = imdb._image_set if image_set is None else image_set
    written = []
    for i in range(imdb.num_images):
        data, im_info, gt, num = (t.unsqueeze(0) for t in loader[i][:4])
        rois, cls_prob, bbox_pred = labeler(data, im_info, gt, num)[:3]
        dets, counts = detect(rois[0], cls_prob[0], bbox_pred[0], im_info[0], class_agnostic,
                              thresh)
        objects = label_objects(dets.cpu().numpy(), counts.cpu().numpy(), imdb.classes)
        width, height = Image.open(imdb.image_path_at(i)).size
        write_label_xml(devkit_out, year, imdb.image_index[i], height, width, objects)
        written.append(len(objects))
    main = os.path.join(devkit_out, "VOC" + year, "ImageSets", "Main")
    os.makedirs(main, exist_ok=True)
    with open(os.path.join(main, image_set + ".txt"), "w") as f:
        for index in imdb.image_index:
            f.write(index + "\n")
    return written
