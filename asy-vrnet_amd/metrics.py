"""Segmentation metrics on the device, with the interfaces of utils_seg/utils_metrics.py: `f_score` (:12-31, called on
every training and validation step, utils/utils_fit.py:78,109,177) and `fast_hist` (:35-44, the per-image confusion
matrix of compute_mIoU, :102).  Each is one or two HIP launches with no host synchronisation; the result stays on the
device until the caller reads it.  per_class_iu, per_class_PA_Recall, per_class_Precision and per_Accuracy (:47-60) work
unchanged on `hist.cpu().numpy()`.  No CPU fallback."""
import torch

from . import hip

MAX_CLASSES = 32              # the seg loss's class cap (SMAXC in csrc/loss.hip)


def f_score(inputs, target, beta=1, smooth=1e-5, threhold=0.5):
    """utils_metrics.py:12-31 (the keyword keeps the reference's spelling): inputs (B, C, H, W) logits, target (B, H, W,
    C+1) one-hot labels.  Per class c < C over all pixels tp = sum t_c [p_c > threhold], fp, fn as the reference;
    returns the mean over c of ((1+b^2) tp + smooth) / ((1+b^2) tp + b^2 fn + fp + smooth) as a 0-d fp32 tensor on the
    logits' device.  The logits must already be at the target's size: the reference's bilinear resize branch (:15-16)
    never runs on this net, whose seg head outputs full resolution."""
    if not (torch.is_tensor(inputs) and inputs.dim() == 4 and torch.is_tensor(target) and target.dim() == 4):
        raise RuntimeError("f_score: expects (B, C, H, W) logits and a (B, H, W, C+1) one-hot target")
    B, C, H, W = inputs.shape
    if not 0 < C <= MAX_CLASSES:
        raise RuntimeError(f"f_score: {C} classes (1..{MAX_CLASSES} supported)")
    if tuple(target.shape) != (B, H, W, C + 1):
        raise RuntimeError(f"f_score: target must be (B, H, W, C+1) = {(B, H, W, C + 1)} for logits {tuple(inputs.shape)} "
                           "(the reference's resize branch, utils_metrics.py:15-16, never runs on this net)")
    if not inputs.is_cuda:
        raise RuntimeError("f_score: the logits must be on a GPU (there is no CPU fallback)")
    x = inputs.detach()
    x = x if (x.is_contiguous() and x.dtype == torch.float32) else x.contiguous().float()
    t = target.detach().to(x.device, torch.float32).contiguous()
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    hip.seg_fscore(x, t, beta, smooth, threhold, out)
    return out.reshape(())


_LABEL_DTYPES = (torch.uint8, torch.int64)


def fast_hist(a, b, n, out=None):
    """utils_metrics.py:35-44: a = labels, b = predictions, tensors of one number of elements (any shape, uint8 or int64)
    on the GPU.  Returns the (n, n) int64 confusion matrix on that device, rows = labels, columns = predictions; with
    `out` ((n, n) int64, contiguous) the counts are added to it in place and `out` is returned, so a whole validation set
    needs one read-back.  Pairs whose label is outside [0, n) are skipped, as the reference does (255 "void" pixels, the
    ignore class n); so are pairs whose prediction is outside [0, n), which the reference would count in another bin."""
    n = int(n)
    if not 0 < n <= MAX_CLASSES:
        raise RuntimeError(f"fast_hist: n = {n} (1..{MAX_CLASSES} supported)")
    if not (torch.is_tensor(a) and torch.is_tensor(b)):
        raise RuntimeError("fast_hist: expects label and prediction tensors")
    if a.dtype not in _LABEL_DTYPES or b.dtype not in _LABEL_DTYPES:
        raise RuntimeError(f"fast_hist: labels and predictions must be uint8 or int64, got {a.dtype} / {b.dtype}")
    if a.numel() != b.numel():
        raise RuntimeError(f"fast_hist: {a.numel()} labels but {b.numel()} predictions")
    if out is not None and (tuple(out.shape) != (n, n) or out.dtype != torch.int64 or not out.is_contiguous()):
        raise RuntimeError(f"fast_hist: out must be a contiguous ({n}, {n}) int64 tensor")
    if not (a.is_cuda and b.is_cuda and a.device == b.device and (out is None or out.device == a.device)):
        raise RuntimeError("fast_hist: the tensors must be on one GPU (there is no CPU fallback)")
    if out is None:
        out = torch.zeros((n, n), dtype=torch.int64, device=a.device)
    hip.confusion_hist(a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1), n, out)
    return out
