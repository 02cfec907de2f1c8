"""File-backed datasets with the reference's names (datasets/cityscapes_Dataset.py,
datasets/gta5_Dataset.py, datasets/synthia_Dataset.py, datasets/crosscity_Dataset.py): PNGs decoded on the
host - by Pillow, SYNTHIA's 16-bit labels by utils/png.py up to the inflate, the NTHU cities' JPEGs by
utils/jpeg.py up to the Huffman decode - everything after the decode - the PNG unfilter of those labels, the
JPEGs' inverse DCT, upsampling and colour conversion, mirror, crop, BICUBIC / NEAREST resize, BGR - mean,
id -> trainId - on the device, byte-exact (utils/preprocess.py png_unfilter / jpeg_reconstruct / resize_image /
resize_label)."""
from .cityscapes_Dataset import City_DataLoader, City_Dataset, Client_dataset, DeviceLoader  # noqa: F401
from .gta5_Dataset import GTA5_DataLoader, GTA5_Dataset  # noqa: F401
from .synthia_Dataset import SYNTHIA_DataLoader, SYNTHIA_Dataset  # noqa: F401
from .crosscity_Dataset import CrossCity_DataLoader, CrossCity_Dataset  # noqa: F401


def build_loader(name, args, training, paths):
    """The loader of dataset `name` ('cityscapes' | 'gta5' | 'synthia' | 'crosscity') over paths = {data_root_path,
    list_path, gt_path}.  SYNTHIA's and a cross-city tree are checked before anything else, so a wrong root is
    reported as such whatever else is missing."""
    from ..hip import MSLError
    key = str(name).lower()
    if key == "cityscapes":
        return City_DataLoader(args, training=training, datasets_path={"Cityscapes": paths})
    if key == "gta5":
        return GTA5_DataLoader(args, training=training, datasets_path=paths)
    if key == "synthia":
        from .synthia_Dataset import check_tree
        check_tree(paths)
        return SYNTHIA_DataLoader(args, training=training, datasets_path=paths)
    if key == "crosscity":
        from .crosscity_Dataset import check_tree
        check_tree(paths)
        return CrossCity_DataLoader(args, training=training, datasets_path=paths)
    raise MSLError(f"no file-backed loader for dataset {name!r} (cityscapes | gta5 | synthia | crosscity)")
