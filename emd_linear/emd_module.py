from cloud_transformers_amd.emd import emdFunction, emdModule  # noqa: F401
from cloud_transformers_amd.emd import EmdWithCountsFunction, emd_distance, emd_with_counts, loss_emd_counts  # noqa: F401
