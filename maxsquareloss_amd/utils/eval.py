"""Segmentation metrics of the reference's `Eval` (utils/eval.py:13-118), confusion matrix on device.

The reference bins `num_class * gt + argmax(pred)` with np.bincount after copying the
prediction and label to the host every iteration (tools/train_source.py:280-283); here
`add_batch(label, pred)` takes the device tensors and runs `msl_confusion_accumulate`
(csrc/eval.hip: fused argmax + exact integer counts), and the matrix only crosses to the host
when a metric is read.  `add_batch_low` is the evaluator's form: from the low-resolution head
logits, upsampling included (msl_predict_up), optionally with the --flip average.  The metric
definitions follow utils/eval.py: per-class accuracy / IoU / precision with NaN for absent classes, nan-means over classes (`ignore_index` slicing),
16/13-class SYNTHIA subsets, and FWIoU as the frequency-weighted sum of the non-NaN IoUs.
"""
import numpy as np
import torch

from .. import hip, ops

# the row names of Print_Every_class_Eval (datasets/cityscapes_Dataset.py:379-400)
name_classes = ['road', 'sidewalk', 'building', 'wall', 'fence', 'pole', 'trafflight', 'traffsign', 'vegetation',
                'terrain', 'sky', 'person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle',
                'unlabeled']

# utils/eval.py:9-11
synthia_set_16 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 15, 17, 18]
synthia_set_13 = [0, 1, 2, 6, 7, 8, 10, 11, 12, 13, 15, 17, 18]
synthia_set_16_to_13 = [0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / den


class Eval:
    def __init__(self, num_class):
        self.num_class = num_class
        self.ignore_index = None
        self.synthia = num_class == 16
        self._dev = None  # int64 [C*C] on the GPU, accumulated by add_batch
        self._host = np.zeros((num_class, num_class))

    # ------------------------------------------------------------------ accumulation
    def add_batch(self, gt_image, pre_image):
        """gt_image: int64 labels [N, H, W] (or [H, W]); pre_image: fp32 logits [N, C, H, W] on
        the GPU (argmax taken on device), same H, W.  Pixels with gt outside [0, C) are skipped."""
        if not (torch.is_tensor(pre_image) and pre_image.is_cuda and pre_image.dim() == 4):
            raise hip.MSLError("Eval.add_batch: expects device logits [N, C, H, W]")
        c = pre_image.size(1)
        if c != self.num_class:
            raise hip.MSLError(f"Eval.add_batch: {c} classes, Eval built for {self.num_class}")
        gt = gt_image.to(device=pre_image.device, dtype=torch.int64).reshape(pre_image.size(0), -1).contiguous()
        pred = pre_image.detach().float().contiguous()
        p = pred.size(2) * pred.size(3)
        if gt.size(1) != p:
            raise hip.MSLError("Eval.add_batch: label and prediction sizes differ")
        if self._dev is None or self._dev.device != pred.device:
            self._dev = torch.zeros(c * c, dtype=torch.int64, device=pred.device)
        lib = hip.load()
        for n in range(pred.size(0)):
            hip.check(lib.msl_confusion_accumulate(pred[n].data_ptr(), gt[n].data_ptr(), c, p,
                                                   self._dev.data_ptr(), None, hip.stream_ptr()),
                      "msl_confusion_accumulate")

    def add_batch_low(self, gt_image, low, out_hw, low_flip=None, images=None, thr=0.95):
        """add_batch from the LOW-resolution logits `low` (1,C,hi,wi) of one image: the class of every
        pixel of out_hw and its matrix cell in one kernel (ops.predict_up), the upsampled prediction
        never written.  With `low_flip` (the mirrored image's low-res logits) the class is the
        evaluator's --flip average (tools/evaluate.py:120-135); without, add_batch's argmax of
        ops.upsample_bilinear(low, out_hw), bit for bit.  `images` (a dict of uint8 buffers,
        ops.image_buffers) also receives that class as images, still in the one launch
        (ops.predict_images; `thr` is the pseudo-label threshold)."""
        if not (torch.is_tensor(low) and low.is_cuda and low.dim() == 4 and low.size(0) == 1):
            raise hip.MSLError("Eval.add_batch_low: expects device logits [1, C, hi, wi]")
        c = low.size(1)
        if c != self.num_class:
            raise hip.MSLError(f"Eval.add_batch_low: {c} classes, Eval built for {self.num_class}")
        gt = gt_image.to(device=low.device, dtype=torch.int64).reshape(-1).contiguous()
        if gt.numel() != int(out_hw[0]) * int(out_hw[1]):
            raise hip.MSLError("Eval.add_batch_low: label and prediction sizes differ")
        if self._dev is None or self._dev.device != low.device:
            self._dev = torch.zeros(c * c, dtype=torch.int64, device=low.device)
        if images is not None:
            ops.predict_images(low, out_hw, low_flip, gt, self._dev, out=images, thr=thr)
        else:
            ops.predict_up(low, out_hw, low_flip, gt, self._dev)

    def add_batch_tta(self, gt_image, entries, out_hw, images=None, thr=0.95):
        """add_batch_low over several low-resolution predictions of one image, fused in one launch
        (ops.predict_tta): `entries` are (low, mirror) pairs, each low (1,C,hi,wi) at its own size - the
        image at some input scale, or that image's mirror.  `images` as add_batch_low
        (ops.predict_tta_images)."""
        entries = list(entries)
        low = entries[0][0] if entries else None
        if not (torch.is_tensor(low) and low.is_cuda and low.dim() == 4 and low.size(0) == 1):
            raise hip.MSLError("Eval.add_batch_tta: expects (device logits [1, C, hi, wi], mirror) entries")
        c = low.size(1)
        if c != self.num_class:
            raise hip.MSLError(f"Eval.add_batch_tta: {c} classes, Eval built for {self.num_class}")
        gt = gt_image.to(device=low.device, dtype=torch.int64).reshape(-1).contiguous()
        if gt.numel() != int(out_hw[0]) * int(out_hw[1]):
            raise hip.MSLError("Eval.add_batch_tta: label and prediction sizes differ")
        if self._dev is None or self._dev.device != low.device:
            self._dev = torch.zeros(c * c, dtype=torch.int64, device=low.device)
        if images is not None:
            ops.predict_tta_images(entries, out_hw, gt, self._dev, out=images, thr=thr)
        else:
            ops.predict_tta(entries, out_hw, gt, self._dev)

    def add_batch_rectified(self, gt_image, low, crop0, crop1, out_hw, segy0):
        """add_batch_low without flip, followed by the reference's Trainer.rectification with the logits of
        its two stylised, magnified crops, in the same launch (ops.predict_rectify)."""
        if not (torch.is_tensor(low) and low.is_cuda and low.dim() == 4 and low.size(0) == 1):
            raise hip.MSLError("Eval.add_batch_rectified: expects device logits [1, C, hi, wi]")
        c = low.size(1)
        if c != self.num_class:
            raise hip.MSLError(f"Eval.add_batch_rectified: {c} classes, Eval built for {self.num_class}")
        gt = gt_image.to(device=low.device, dtype=torch.int64).reshape(-1).contiguous()
        if gt.numel() != int(out_hw[0]) * int(out_hw[1]):
            raise hip.MSLError("Eval.add_batch_rectified: label and prediction sizes differ")
        if self._dev is None or self._dev.device != low.device:
            self._dev = torch.zeros(c * c, dtype=torch.int64, device=low.device)
        ops.predict_rectify(low, crop0, crop1, out_hw, segy0, gt, self._dev)

    def reset(self):
        self._host = np.zeros((self.num_class,) * 2)
        if self._dev is not None:
            self._dev.zero_()

    @property
    def confusion_matrix(self):
        """[gt][pred] counts as float64 (the reference's dtype); syncs the device matrix."""
        m = self._host
        if self._dev is not None:
            m = m + self._dev.view(self.num_class, self.num_class).cpu().numpy().astype(np.float64)
        return m

    @confusion_matrix.setter
    def confusion_matrix(self, value):
        self._host = np.asarray(value, dtype=np.float64).copy()
        if self._dev is not None:
            self._dev.zero_()

    # ------------------------------------------------------------------ metrics
    def _reduce(self, per_class, out_16_13):
        if self.synthia:
            return np.nanmean(per_class[:self.ignore_index]), np.nanmean(per_class[synthia_set_16_to_13])
        if out_16_13:
            return np.nanmean(per_class[synthia_set_16]), np.nanmean(per_class[synthia_set_13])
        return np.nanmean(per_class[:self.ignore_index])

    def Pixel_Accuracy(self):
        m = self.confusion_matrix
        total = m.sum()
        if total == 0:
            print("Attention: pixel_total is zero!!!")
            return 0
        return np.trace(m) / total

    def _iou(self, m):
        d = np.diag(m)
        return _ratio(d, m.sum(axis=1) + m.sum(axis=0) - d)

    def Mean_Pixel_Accuracy(self, out_16_13=False):
        m = self.confusion_matrix
        return self._reduce(_ratio(np.diag(m), m.sum(axis=1)), out_16_13)

    def Mean_Intersection_over_Union(self, out_16_13=False):
        return self._reduce(self._iou(self.confusion_matrix), out_16_13)

    def Mean_Precision(self, out_16_13=False):
        m = self.confusion_matrix
        return self._reduce(_ratio(np.diag(m), m.sum(axis=0)), out_16_13)

    def Frequency_Weighted_Intersection_over_Union(self, out_16_13=False):
        m = self.confusion_matrix
        fw = m.sum(axis=1) * self._iou(m)
        total = m.sum()

        def part(v):
            return float(v[~np.isnan(v)].sum()) / total

        if self.synthia:
            return part(fw), part(fw[synthia_set_16_to_13])
        if out_16_13:
            return part(fw[synthia_set_16]), part(fw[synthia_set_13])
        return part(fw)

    def Print_Every_class_Eval(self, out_16_13=False):
        """The per-class table of utils/eval.py:90-106, character for character: accuracy, IoU,
        precision, label share and prediction share in percent (round(., 2), 'nan' for an absent
        class).  As there, out_16_13 shortens only the IoU column to the 16 SYNTHIA classes while the
        row names and the other columns keep running over the first 16 indices."""
        m = self.confusion_matrix
        d, rows, cols, total = np.diag(m), m.sum(axis=1), m.sum(axis=0), m.sum()
        iou = self._iou(m)
        columns = [_ratio(d, rows), iou[synthia_set_16] if out_16_13 else iou, _ratio(d, cols),
                   _ratio(rows, total), _ratio(cols, total)]
        print('===>Everyclass:\t' + 'MPA\t' + 'MIoU\t' + 'PC\t' + 'Ratio\t' + 'Pred_Retio')
        for i in range(len(columns[1])):
            cells = [str(round(v[i] * 100, 2)) if not np.isnan(v[i]) else 'nan' for v in columns]
            print('===>' + name_classes[i] + ':\t' + '\t'.join(cells))
