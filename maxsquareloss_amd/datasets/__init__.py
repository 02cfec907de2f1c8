"""File-backed datasets with the reference's names (datasets/cityscapes_Dataset.py,
datasets/gta5_Dataset.py): PNGs decoded by Pillow on the host, everything after the decode -
mirror, crop, BICUBIC / NEAREST resize, BGR - mean, id -> trainId - on the device, byte-exact
(utils/preprocess.py resize_image / resize_label)."""
from .cityscapes_Dataset import City_DataLoader, City_Dataset, Client_dataset, DeviceLoader  # noqa: F401
from .gta5_Dataset import GTA5_DataLoader, GTA5_Dataset  # noqa: F401


def build_loader(name, args, training, paths):
    """The loader of dataset `name` ('cityscapes' | 'gta5') over paths = {data_root_path, list_path,
    gt_path}; SYNTHIA's 16-bit label PNGs need imageio's FreeImage plugin and stay out."""
    from ..hip import MSLError
    key = str(name).lower()
    if key == "cityscapes":
        return City_DataLoader(args, training=training, datasets_path={"Cityscapes": paths})
    if key == "gta5":
        return GTA5_DataLoader(args, training=training, datasets_path=paths)
    if key == "synthia":
        raise MSLError("file-backed SYNTHIA is not supported: its 16-bit label PNGs need imageio's FreeImage "
                       "plugin, which this package does not depend on; use --source_dataset gta5, or leave the "
                       "data paths unset for the synthetic loaders")
    raise MSLError(f"no file-backed loader for dataset {name!r} (cityscapes | gta5)")
