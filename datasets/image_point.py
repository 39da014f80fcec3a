from cloud_transformers_amd.data.image_point import (IMAGENET_MEAN, IMAGENET_STD, ImageToPoint, pil_loader, read_ply,  # noqa: F401
                                                     resample_pcd)
