"""Drop-in for ``pldepth/data/dao/dao_meta.py``: the DAO of a dataset type, rooted at the
``[DATA] *_ROOT_PATH`` key of the config (dao_meta.py:9-22)."""
from ..io_utils import Dataset
from .diode import DIODETFDataAccessObject
from .hr_wsi import HRWSITFDataAccessObject
from .ibims import IbimsTFDataAccessObject
from .sintel import SintelTFDataAccessObject
from .tum import TUMTFDataAccessObject


def get_dao_for_dataset_type(dataset_type, config, model_input_shape, seed=0):
    if dataset_type == Dataset.IBIMS:
        dao = IbimsTFDataAccessObject(config["DATA"]["IBIMS_ROOT_PATH"], model_input_shape)
    elif dataset_type == Dataset.DIODE:
        dao = DIODETFDataAccessObject(config["DATA"]["DIODE_ROOT_PATH"], model_input_shape)
    elif dataset_type == Dataset.SINTEL:
        dao = SintelTFDataAccessObject(config["DATA"]["SINTEL_ROOT_PATH"], model_input_shape)
    elif dataset_type == Dataset.TUM:
        dao = TUMTFDataAccessObject(config["DATA"]["TUM_ROOT_PATH"], model_input_shape)
    elif dataset_type == Dataset.HR_WSI:
        dao = HRWSITFDataAccessObject(config["DATA"]["HR_WSI_ROOT_PATH"], model_input_shape, seed)
    else:
        raise NotImplementedError(
            "Model evaluation currently does not support dataset type '{}'.".format(dataset_type))
    return dao
