"""`datasets.grnet_completion` (reference datasets/grnet_completion.py:344-512): the ShapeNet completion loader."""
from cloud_transformers_amd.data.completion import (Compose, Dataset, DatasetSubset, RandomMirrorPoints, RandomSamplePoints,  # noqa: F401
                                                    ShapeNetDataLoader, ToTensor, collate_fn, read_pcd)
