"""Host-side data preparation of the MHCT pipelines: voxel-grid subsampling, the dataset classes of the
reference's loaders and their augmentations.  CPU only — numpy in, numpy / torch CPU tensors out — except the device
protocols (s3dis_kpconv and the other *_device loaders) and subsampling.compute_device, which keep tensors on a HIP device."""
