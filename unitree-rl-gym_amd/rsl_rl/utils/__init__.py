from .utils import capture_without_gc, split_and_pad_trajectories, unpad_trajectories
