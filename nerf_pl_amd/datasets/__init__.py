"""`datasets/__init__.py` of the reference: Blender scenes, loaded on the GPU.  LLFF (`datasets/llff.py`: JPEG files, COLMAP
poses) is not built."""
from .blender import BlenderDataset

dataset_dict = {'blender': BlenderDataset}
