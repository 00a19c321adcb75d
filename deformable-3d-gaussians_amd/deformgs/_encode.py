"""What the two device image writers (png_gpu.py, jpeg_gpu.py) share: the checks every batch of frames must pass,
the fetch of the packed streams to the host and the writing of the finished files."""
import torch


def check_frames(frames, cpu_hint=""):
    """frames must be a uint8 tensor on the device; the shape is the caller's to check."""
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f"encode_frames takes a device uint8 tensor, got {type(frames).__name__}")
    if not frames.is_cuda:
        raise ValueError("encode_frames takes a device (HIP) tensor; got a CPU tensor" + cpu_hint)
    if frames.dtype != torch.uint8:
        raise ValueError(f"encode_frames takes uint8 frames, got {frames.dtype}")


def fetch_spans(offsets, lengths):
    """Device int64 offsets and lengths -> ([(offset, length)] on the host, where the last stream ends). One copy."""
    where = torch.stack([offsets, lengths]).cpu().tolist()
    return list(zip(*where)), where[0][-1] + where[1][-1]


def fetch_bytes(packed, total):
    """The first `total` bytes of the device tensor as bytes. One copy."""
    return packed[:total].cpu().numpy().tobytes()


def write_files(paths, files):
    """Writes files[i] to paths[i]."""
    paths = list(paths)
    if len(paths) != len(files):
        raise ValueError(f"write_frames: {len(paths)} paths for {len(files)} frames")
    for path, data in zip(paths, files):
        with open(path, "wb") as f:
            f.write(data)
