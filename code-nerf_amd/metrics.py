"""Evaluation metrics of the reference's optimisation loop (src/optimizer.py).

``psnr(mse) = -10 log10(mse)`` (src/optimizer.py:163,169, src/trainer.py:99).

``ssim_legacy`` restates what ``skimage.metrics.structural_similarity(a, b,
multichannel=True)`` computes for the float images the reference passes
(src/optimizer.py:156; skimage is not installed here, so this is PARITY
UNPINNED -- it follows skimage's published algorithm as of the 0.18/0.19
series the reference's environment resolves to): per channel, 7x7 uniform
window (scipy.ndimage.uniform_filter, mode 'reflect'), sample covariance
(N/(N-1)), K1 = 0.01, K2 = 0.03, data_range = 2 (the float dtype range
(-1, 1) skimage infers when none is given), mean over the image cropped by
(win-1)/2 on each side, then the mean over channels; float64 throughout.

``image_metrics`` computes both numbers on the device (cn_image_metrics,
csrc/metrics.hip): the mean of the chunk MSEs ``psnr`` takes and
``ssim_legacy``'s value, for any number of views, without a host
synchronisation.
"""
import numpy as np

_ws = {}        # (device index, stream) -> workspace tensor of cn_image_metrics


def image_metrics(img, gt, H, W, chunk, out=None, chunk_mse=None):
    """(mse, ssim) of rendered against target views, on the device.

    img, gt: float32 device tensors (V, H*W, 3), or (H*W, 3) for one view,
    pixel = row * W + col.  Returns a (V, 2) float64 device tensor, queued on
    the current stream (no host synchronisation): column 0 is the mean over
    chunks of ``chunk`` rays of the chunk-mean squared error -- ``psnr`` of it
    is the loop's PSNR -- and column 1 is ``ssim_legacy``'s value.  ``out``: a
    (V, 2) float64 contiguous device tensor to write instead, e.g. rows of a
    larger result buffer read back once.  ``chunk_mse``: a (V, ceil(H*W/chunk))
    float64 contiguous device tensor that receives the chunk means.
    """
    import torch

    from . import _lib
    L = _lib.lib()                      # HipUnavailable without a device
    if img.dim() == 2:
        img, gt = img[None], gt[None]
    V = img.shape[0]
    if img.shape != (V, H * W, 3) or gt.shape != img.shape:
        raise ValueError(f"image_metrics: expected two (V, {H * W}, 3) tensors, got {tuple(img.shape)} and "
                         f"{tuple(gt.shape)}")
    if img.dtype != torch.float32 or gt.dtype != torch.float32 or not img.is_cuda or gt.device != img.device:
        raise ValueError("image_metrics: img and gt must be float32 tensors on one HIP device")
    img, gt = img.contiguous(), gt.contiguous()
    if out is None:
        out = torch.empty(V, 2, dtype=torch.float64, device=img.device)
    elif (out.shape != (V, 2) or out.dtype != torch.float64 or out.device != img.device
          or not out.is_contiguous()):
        raise ValueError(f"image_metrics: out must be a contiguous ({V}, 2) float64 tensor on {img.device}")
    if chunk_mse is not None and (chunk_mse.dtype != torch.float64 or chunk_mse.device != img.device
                                  or not chunk_mse.is_contiguous()
                                  or chunk_mse.shape != (V, -(-H * W // max(int(chunk), 1)))):
        raise ValueError("image_metrics: chunk_mse must be a contiguous (V, ceil(H*W/chunk)) float64 device tensor")
    nbytes = L.cn_image_metrics_ws_bytes(H, W, V, chunk)
    stream = _lib.stream_ptr(img.device)
    # one workspace per stream: calls queued on one stream run in order
    key = (img.device.index, stream.value)
    ws = _ws.get(key)
    if nbytes and (ws is None or ws.numel() < nbytes):
        ws = _ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    _lib.check(L.cn_image_metrics(_lib.ptr(img), _lib.ptr(gt), H, W, V, chunk, _lib.ptr(out), _lib.ptr(chunk_mse),
                                  _lib.ptr(ws), stream), "cn_image_metrics")
    return out


def psnr(mse):
    return -10.0 * np.log(mse) / np.log(10.0)


def _ssim_channel(x, y, win=7, K1=0.01, K2=0.03, data_range=2.0):
    from scipy.ndimage import uniform_filter
    npix = win * win
    cov_norm = npix / (npix - 1.0)
    ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
    uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    pad = (win - 1) // 2
    return S[pad:-pad, pad:-pad].mean()


def ssim_legacy(img1, img2, win=7, data_range=2.0):
    """img1, img2: (H, W, C) float arrays -> mean SSIM over channels."""
    a = np.asarray(img1, dtype=np.float64)
    b = np.asarray(img2, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("ssim_legacy expects two (H, W, C) images of the same shape")
    return float(np.mean([_ssim_channel(a[..., c], b[..., c], win, data_range=data_range)
                          for c in range(a.shape[-1])]))
