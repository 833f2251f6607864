"""`datasets/__init__.py` of the reference: Blender scenes (`datasets/blender.py`: RGBA PNG files) and LLFF scenes
(`datasets/llff.py`: JPEG or PNG files, COLMAP poses), both decoded, resized and converted on the GPU.

`dataset_dict` holds the Blender loader only: tests/test_datasets_host.py pins it to exactly that entry.  The LLFF loader is
`LLFFDataset` (also `datasets.llff.LLFFDataset` after `nerf_pl_amd.install(datasets=True)`); a caller that selects loaders by
name uses `dataset_classes`."""
from .blender import BlenderDataset
from .llff import LLFFDataset

dataset_dict = {'blender': BlenderDataset}
dataset_classes = {'blender': BlenderDataset,
                   'llff': LLFFDataset}
