"""`utils.pcd_utils` (reference utils/pcd_utils.py:5-51)."""
from cloud_transformers_amd.data.completion import partial_postproces  # noqa: F401
from cloud_transformers_amd.metrics import resample_pcd, sphere_noise  # noqa: F401
