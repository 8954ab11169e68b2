"""NaN-guarded device layouts for the tests that drive kernels through raw pointers: every tensor is a view into one
NaN-filled buffer, so a write outside a tensor shows as a guard element that is no longer NaN."""
import torch

NAN = float("nan")


def guarded_tensors(sizes, gap=9):
    """tensors carved out of one NaN-filled buffer with NaN gaps around each; even-numbered ones 16-byte aligned (float4
    path), odd-numbered ones one float off (scalar path)"""
    total = sum(sizes) + (gap + 4) * (len(sizes) + 1)
    buf = torch.full((total,), NAN, device="cuda")
    views, off = [], gap
    for k, n in enumerate(sizes):
        off = (off + 3) // 4 * 4 + k % 2
        views.append(buf[off:off + n])
        off += n + gap
    return buf, views


def guards_are_nan(buf, views):
    """Is every element of buf outside the views still NaN?"""
    mask = torch.ones_like(buf, dtype=torch.bool)
    for vw in views:
        o = (vw.data_ptr() - buf.data_ptr()) // 4
        mask[o:o + vw.numel()] = False
    return bool(torch.isnan(buf[mask]).all())
