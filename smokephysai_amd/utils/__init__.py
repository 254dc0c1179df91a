from .data_loader import SyntheticSmokeDataset, SyntheticSmokeDataset3D, create_data_loaders
from .distributed import init_distributed, shard_range, wrap_ddp

__all__ = ["SyntheticSmokeDataset", "SyntheticSmokeDataset3D", "create_data_loaders", "init_distributed", "shard_range", "wrap_ddp",
           "SmokeVisualizer"]


def __getattr__(name):
    if name == "SmokeVisualizer":          # on first use: the module imports matplotlib and picks its backend
        from .visualization import SmokeVisualizer
        return SmokeVisualizer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
