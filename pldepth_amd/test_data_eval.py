"""Test-set evaluation entry point (in place of pldepth/test_data_eval.py:30-104, which evaluates
a checkpoint at a hard-coded path on HR-WSI): every number the method is judged by, for a trained
model on any of the datasets, as one process on one GPU.

    python -m pldepth_amd.test_data_eval --model_name ff_effnet --load_model_path w.h5 \\
        --dataset ibims --data_path /data/ibims --input_size 448 --batch_size 32

Data: ``--data_path`` is the root the dataset's DAO reads (data/dao/dao_meta.py; default: the
config's ``[DATA] <NAME>_ROOT_PATH``); ``--data_npz`` loads arrays instead (``val_imgs`` /
``val_gts``, else ``imgs`` / ``gts``: [N, H, W, 3] in [0, 1] and [N, H, W]); with neither a
seeded synthetic set of two batches is evaluated (``synthetic_eval_set``: the training entry
point's synthetic set with an occlusion boundary in every depth map).

Printed, one ``name value`` line each:
  ordinal_pair_error   over ``--val_rankings_per_img`` random point pairs per image at
                       ``--equality_threshold`` (GenericHourglassPairRelationDataProvider +
                       active_learning.metrics.ordinal_pair_error)
  ranking_loss         ``model.evaluate`` over the batches of
                       GenericHourglassRankingDataProvider (100 rankings of ``--ranking_size``)
  test_error, ndcg_200, depth_boundary_metric, depth_completeness
                       the reference script's own metrics (test_data_eval.py:94-102); the first
                       needs at least 10,000 pixels per image and the second 224 x 224, as in the
                       training entry point's test pass
The relation sign is inverted for every dataset but HR-WSI (pl_hourglass.py:26-27: there larger
values are closer). ``--cache`` keeps the pair and ranking tables as ``.npy`` files under that
prefix, under the reference's file names. wandb logging is not part of this build.
"""
import click
import numpy as np

from .active_learning.metrics import (calc_depth_metrics, calc_err, dcg_metric,
                                      ordinal_pair_error)
from .kernels import EDGE_MAX_DIM
from .data.io_utils import Dataset, get_dataset_type_by_name
from .data.providers.generic_ranking_provider import (GenericHourglassPairRelationDataProvider,
                                                      GenericHourglassRankingDataProvider)
from .losses.losses_meta import DepthLossType
from .losses.nll_loss import HourglassNegativeLogLikelihood
from .models.models_meta import ModelParameters, get_model_type_by_name
from .models.PLDepthNet import get_pl_depth_net
from .util.env import get_config


def synthetic_eval_set(n, h, w, seed=0):
    """The training entry point's seeded synthetic images with depth maps that have what test
    sets have and its smooth fields lack, an occlusion boundary: the smooth field fills the far
    half of the 8-bit range and one rectangle per image sits in front of it at the nearest
    value. The step of at least half the range is a Canny edge of every map, so the depth-edge
    metrics (nan for a map without edges) are defined."""
    from .PLDepth import synthetic_hrwsi
    imgs, gts, _ = synthetic_hrwsi(n, h, w, seed)
    gts = np.round(127 * gts) / np.float32(255)
    rng = np.random.default_rng(seed)
    for g in gts:
        bh, bw = rng.integers(h // 4, h // 2 + 1), rng.integers(w // 4, w // 2 + 1)
        y0, x0 = rng.integers(1, h - bh), rng.integers(1, w - bw)
        g[y0:y0 + bh, x0:x0 + bw] = 1.0
    return imgs, gts.astype(np.float32)


def load_test_set(dataset_type, data_path, data_npz, shape, batch_size, seed, config):
    """(imgs [N, H, W, 3], gts [N, H, W]) float32 host arrays."""
    if data_npz:
        with np.load(data_npz, allow_pickle=False) as z:
            pre = "val_" if "val_imgs" in z.files else ""
            return z[pre + "imgs"].astype(np.float32), z[pre + "gts"].astype(np.float32)
    if data_path:
        from .data.dao.dao_meta import get_dao_for_dataset_type
        config["DATA"][dataset_type.name + "_ROOT_PATH"] = data_path
        dao = get_dao_for_dataset_type(dataset_type, config, shape, seed)
        imgs, gts = dao.get_test_dataset(zip_ds=False)
        return imgs, gts.reshape(gts.shape[:3])
    return synthetic_eval_set(2 * batch_size, shape[0], shape[1], seed + 1)


def evaluate(model, imgs, gts, model_params, dataset_type, config, use_cache, out=print):
    """Runs every metric and hands ``name value`` lines to ``out``; returns {name: value}."""
    seed = model_params.get_parameter("seed")
    L = model_params.get_parameter("ranking_size")
    B = model_params.get_parameter("batch_size")
    H, W = imgs.shape[1:3]
    invert = dataset_type != Dataset.HR_WSI
    res = {}

    def report(name, value):
        res[name] = float(value)
        out(f"{name} {res[name]:.6f}")

    pair_prov = GenericHourglassPairRelationDataProvider(
        model_params, seed, invert, threshold=model_params.get_parameter("equality_threshold"),
        save_pairs_on_disk=use_cache, config=config)
    pair_ds = pair_prov.provide_test_dataset((imgs, gts))
    report("ordinal_pair_error", ordinal_pair_error(model, pair_ds.images, pair_ds.targets)[0])
    rank_prov = GenericHourglassRankingDataProvider(
        model_params, L, seed, invert, save_rankings_on_disk=use_cache, config=config)
    rank_ds = rank_prov.provide_test_dataset((pair_ds.images, gts))
    report("ranking_loss", model.evaluate(rank_ds.batch(B)))
    test_img, test_gt = pair_ds.images, np.asarray(gts, np.float32)[..., None]
    if H * W >= 2 * 5000:
        report("test_error", calc_err(model, test_img, test_gt, img_size=(H, W)))
    if H * W >= 224 * 224:
        report("ndcg_200", dcg_metric(model, test_img, test_gt, list_size=200))
    if max(H, W) <= EDGE_MAX_DIM:
        d_boundary, d_comp = calc_depth_metrics(model, test_img, test_gt)
        report("depth_boundary_metric", d_boundary)
        report("depth_completeness", d_comp)
    return res


@click.command()
@click.option('--model_name', default='ff_effnet', help='Backbone model',
              type=click.Choice(['ff_redweb', 'ff_effnet'], case_sensitive=False))
@click.option('--load_model_path', default='', help='weights to evaluate (Keras .h5 or .npz)')
@click.option('--dataset', default='HR-WSI', help='HR-WSI, IBIMS, SINTEL, DIODE or TUM')
@click.option('--data_path', default='', help="root of the dataset's files")
@click.option('--data_npz', default='', help='npz with (val_)imgs / (val_)gts arrays')
@click.option('--input_size', default=224, type=click.INT)
@click.option('--batch_size', default=6)
@click.option('--seed', default=0)
@click.option('--ranking_size', default=5, help='Number of elements per evaluated ranking')
@click.option('--val_rankings_per_img', default=100, help='Ordinal pairs per image')
@click.option('--equality_threshold', default=0.03, type=click.FLOAT)
@click.option('--cache', default='', help='cache path prefix for the pair / ranking tables')
def eval_model(model_name, load_model_path, dataset, data_path, data_npz, input_size, batch_size,
               seed, ranking_size, val_rankings_per_img, equality_threshold, cache):
    np.random.seed(seed)
    config = get_config()
    if cache:
        config["DATA"]["CACHE_PATH_PREFIX"] = cache
    dataset_type = get_dataset_type_by_name(dataset)
    model_params = ModelParameters()
    for key, value in [("model_type", get_model_type_by_name(model_name)),
                       ("dataset", dataset_type), ("ranking_size", ranking_size),
                       ("rankings_per_image", val_rankings_per_img),
                       ("val_rankings_per_img", val_rankings_per_img),
                       ("batch_size", batch_size), ("seed", seed),
                       ("equality_threshold", equality_threshold),
                       ("loss_type", DepthLossType.NLL)]:
        model_params.set_parameter(key, value)
    shape = [input_size, input_size, 3]
    model, preprocess_fn = get_pl_depth_net(model_params, shape)
    # evaluate() needs the loss only: no optimizer or training step is set up
    model.loss = HourglassNegativeLogLikelihood(ranking_size=ranking_size, batch_size=batch_size)
    if load_model_path:
        model.load_weights(load_model_path)
    imgs, gts = load_test_set(dataset_type, data_path, data_npz, shape, batch_size, seed, config)
    print(f"{dataset_type.value}: {len(imgs)} images of {imgs.shape[1]} x {imgs.shape[2]}")
    evaluate(model, preprocess_fn(imgs), gts, model_params, dataset_type, config, bool(cache))
    return 0


if __name__ == "__main__":
    eval_model()
