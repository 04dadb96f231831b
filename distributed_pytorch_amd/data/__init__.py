from .cifar import (MEAN, NUM_CLASSES, STD, DeviceLoader, ImageSet, ShardSampler, get_datasets,  # noqa: F401
                    load_cifar10, load_cifar100, synthetic_cifar)
