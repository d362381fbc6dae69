"""Frame-once view of frame-stacked observations (pure numpy).

A frame-stacking environment (``AtariEnv._warp``, ``SyntheticAtariEnv`` with
``frame_stack=True``) returns the last C frames at every step, so C - 1 of
the C channels of row r + 1 repeat row r.  A ``LocalBuffer`` block — rows of
consecutive observations of one episode, the carried burn-in prefix included
— is therefore described completely by its first stack plus one new frame
per further row: rows + C - 1 frames instead of rows * C.
``GpuReplayBuffer`` stores that in its ``replay_frame_dedup`` mode and the
gather kernel rebuilds the stacks.
"""

import numpy as np


def frames_from_stacked(obs: np.ndarray, out: np.ndarray = None) -> np.ndarray:
    """(rows, C, H, W) -> (rows + C - 1, H, W): ``obs[0, :C-1]`` followed by
    ``obs[:, C-1]``, one frame per row.  Defined for any input; lossless
    exactly when ``is_frame_stack(obs)``.  ``out``, if given, receives the
    frames (e.g. a pinned staging buffer viewed (rows + C - 1, H, W)), so
    the only copy made is the output itself."""
    rows, C = obs.shape[0], obs.shape[1]
    if out is None:
        out = np.empty((rows + C - 1,) + obs.shape[2:], dtype=obs.dtype)
    assert out.shape == (rows + C - 1,) + obs.shape[2:], out.shape
    out[:C - 1] = obs[0, :C - 1]
    out[C - 1:] = obs[:, C - 1]
    return out


def stacked_from_frames(frames: np.ndarray, C: int) -> np.ndarray:
    """The inverse: (rows + C - 1, H, W) -> (rows, C, H, W) with
    ``out[r, c] = frames[r + c]``."""
    rows = frames.shape[0] - (C - 1)
    assert rows >= 1, "need at least C frames"
    out = np.empty((rows, C) + frames.shape[1:], dtype=frames.dtype)
    for c in range(C):
        out[:, c] = frames[c:c + rows]
    return out


def is_frame_stack(obs: np.ndarray) -> bool:
    """True when every row is the previous one rolled by one frame — the
    invariant under which frames_from_stacked / stacked_from_frames round
    trip."""
    return bool(np.array_equal(obs[1:, :-1], obs[:-1, 1:]))
