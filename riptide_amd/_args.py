"""Argument plumbing of the device layer (engine.py and the modules on top of
it): which device, which stream, and the checks of the tensors every wrapper
takes.  Each message exists once, here."""
import contextlib
import ctypes


def resolve_device(device):
    """torch.device("cuda", index) of None (the current device), an int or a
    torch.device."""
    import torch
    if isinstance(device, torch.device):
        device = device.index
    return torch.device("cuda", torch.cuda.current_device() if device is None else int(device))


def stream_on(device, stream=None):
    """The stream a call is queued on: `stream`, or the device's current one."""
    import torch
    return stream if stream is not None else torch.cuda.current_stream(device)


@contextlib.contextmanager
def stream_scope(device, stream=None):
    """Enter `device` and stream_on(device, stream), so that allocations happen
    there; yields (stream, its raw handle)."""
    import torch
    s = stream_on(device, stream)
    with torch.cuda.device(device), torch.cuda.stream(s):
        yield s, ctypes.c_void_p(s.cuda_stream)


def batch_rows(data):
    """(data as [B, N], B, N, squeezed) of a batch argument, float32 [N] or
    [B, N] on a device with unit sample stride; squeezed says it was [N].
    Whether rows may overlap is the caller's rule."""
    import torch
    squeezed = data.dim() == 1
    if squeezed:
        data = data.unsqueeze(0)
    if data.dim() != 2 or data.dtype != torch.float32 or data.device.type != "cuda" or data.stride(1) != 1:
        raise ValueError("data must be float32 [B, N] device rows with unit stride")
    return data, data.shape[0], data.shape[1], squeezed


def checked_out(out, shape, dtype, device, message, bad=None):
    """An `out` argument: allocated `shape` when None, else ValueError(message)
    unless it is a contiguous `dtype` tensor of exactly `shape` on `device`.
    A caller whose rows may be strided or longer passes its own rule as
    bad(out)."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if bad(out) if bad is not None else (out.dtype != dtype or out.device != device or not out.is_contiguous()
                                         or tuple(out.shape) != tuple(shape)):
        raise ValueError(message)
    return out


def check_workspace(workspace, need, device, whose):
    """ValueError unless workspace is a contiguous uint8 tensor of at least
    `need` bytes on `device` (described as "the {whose}'s device")."""
    import torch
    if (workspace is None or workspace.dtype != torch.uint8 or workspace.device != device
            or not workspace.is_contiguous() or workspace.numel() < need):
        raise ValueError(f"workspace must be a contiguous uint8 tensor of >= {need} bytes on the {whose}'s device")


def checked_workspace(workspace, need, device, whose, floor=0):
    """A `workspace` argument: max(need, floor) bytes allocated when None (the
    floor is the caller's own), else checked by check_workspace."""
    import torch
    if workspace is None:
        return torch.empty(max(need, floor), dtype=torch.uint8, device=device)
    check_workspace(workspace, need, device, whose)
    return workspace
