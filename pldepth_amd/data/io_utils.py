"""Dataset-name dispatch (mirrors pldepth/data/io_utils.py:4-25): the names the drivers accept.

Every name has a data-access object (pldepth_amd.data.dao.dao_meta.get_dao_for_dataset_type):
HR-WSI for training, validation and test, the others (Ibims, Sintel, DIODE, TUM) for test-set
evaluation only, as in the reference.
"""
from ..models.models_meta import StringEnum


class Dataset(StringEnum):
    HR_WSI = "HR-WSI"
    IBIMS = "IBIMS"
    SINTEL = "SINTEL"
    DIODE = "DIODE"
    TUM = "TUM"


_ALIASES = {"hr_wsi": Dataset.HR_WSI}


def get_dataset_type_by_name(dataset_name):
    """io_utils.py:12-25: case-insensitive match on the enum values (plus 'hr_wsi')."""
    key = dataset_name.lower()
    for d in Dataset:
        if key == d.value.lower():
            return d
    if key in _ALIASES:
        return _ALIASES[key]
    raise ValueError("Unknown dataset name: {}".format(dataset_name))
