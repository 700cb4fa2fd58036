"""Active-learning experiment (mirrors pldepth/run_scripts/active_PLDepth.py — same click flags).

    python -m pldepth_amd.run_scripts.active_PLDepth --batch_size 4 --epochs 2 --ds_size 64

Base training exactly as ``pldepth_amd.PLDepth`` sets it up (the reference's lines 71-158: SGDR
with lr_decay 0.5 over ``epochs + 6``), then the active rounds of lines 160-185
(``run_active_rounds``): every pool image is predicted, ``active_learning_data_provider`` selects
16 x 16 pixels per image and lets the oracle rank them, and the model fits one more epoch on
those rankings. The reference leaves its six-round loop with a ``break`` after the first round;
so does this.

Data: the HR-WSI trees named by ``[DATA] HR_WSI_3K_PATH`` / ``HR_WSI_POOL_PATH`` of the config
(util/env.py), read through the HR-WSI DAO; without them a seeded synthetic HR-WSI-shaped set
(PLDepth.synthetic_hrwsi). wandb is optional (active_learning_method.py); mlflow is not used.
"""
import click
import numpy as np

from ..PLDepth import synthetic_hrwsi
from ..active_learning.active_learning_method import active_learning_data_provider
from ..active_learning.metrics import calc_err
from ..data.providers.hourglass_provider import HourglassLargeScaleDataProvider
from ..data.sampling import (InformationScoreBasedSampling, PurelyMaskedRandomSamplingStrategy,
                             ThresholdedMaskedRandomSamplingStrategy)
from ..losses.losses_meta import DepthLossType
from ..losses.nll_loss import HourglassNegativeLogLikelihood
from ..models.models_meta import ModelParameters, get_model_type_by_name
from ..models.PLDepthNet import get_pl_depth_net
from ..optimizers import Adam
from ..util.env import init_env
from ..util.training_utils import LearningRateLoggingCallback, SGDRScheduler, TerminateOnNaN

ACTIVE_ROUNDS = 6   # active_PLDepth.py:171
ACTIVE_SPLIT = 16   # active_PLDepth.py:176


def run_active_rounds(model, pool_imgs, pool_gts, val=None, batch_size=4, ranking_size=3,
                      epochs=0, callbacks=None, schedule=None, split_num=ACTIVE_SPLIT,
                      steps_per_epoch=None, img_size=None, verbose=1):
    """active_PLDepth.py:170-185 on arrays: pool_imgs [N, H, W, 3], pool_gts [N, H, W(, 1)],
    val = validation batches or None. Returns the datasets of the rounds that ran (one: the
    reference's loop ends with a ``break``)."""
    n = len(pool_imgs)
    if schedule is not None:
        schedule.steps_per_epoch = n / batch_size
    img_size = list(img_size) if img_size is not None else list(np.shape(pool_imgs)[1:4])
    rounds = []
    for i in range(ACTIVE_ROUNDS):
        active_train_ds = active_learning_data_provider(pool_imgs, pool_gts, model,
                                                        batch_size=batch_size,
                                                        ranking_size=ranking_size,
                                                        split_num=split_num, img_size=img_size)
        rounds.append(active_train_ds)
        print("fit active sampled data")
        model.fit(x=active_train_ds, initial_epoch=epochs + i, epochs=epochs + i + 1,
                  steps_per_epoch=steps_per_epoch or int(n / batch_size), validation_data=val,
                  verbose=verbose, callbacks=callbacks)
        break
    return rounds


@click.command()
@click.option('--model_name', default='ff_effnet', help='Backbone model',
              type=click.Choice(['ff_redweb', 'ff_effnet'], case_sensitive=False))
@click.option('--epochs', default=50)
@click.option('--batch_size', default=4)
@click.option('--seed', default=0)
@click.option('--ranking_size', default=3, help='Number of elements per training ranking')
@click.option('--rankings_per_image', default=100,
              help='Number of rankings per image for training')
@click.option('--initial_lr', default=0.01, type=click.FLOAT)
@click.option('--equality_threshold', default=0.03, type=click.FLOAT)
@click.option('--model_checkpoints', default=False, type=click.BOOL)
@click.option('--load_model_path', default='', help='Specify the path to a model to load')
@click.option('--augmentation', default=True, type=click.BOOL)
@click.option('--warmup', default=0, type=click.INT)
@click.option('--sampling_type', default=1, type=click.INT)
@click.option('--lr_multi', default=0.25, type=click.FLOAT)
@click.option('--ds_size', default=None, type=click.INT)
def perform_pldepth_experiment(model_name, epochs, batch_size, seed, ranking_size,
                               rankings_per_image, initial_lr, equality_threshold,
                               model_checkpoints, load_model_path, augmentation, warmup,
                               sampling_type, lr_multi, ds_size):
    config = init_env(experiment_name='run1', autolog_freq=1, seed=seed)
    model_params = ModelParameters()
    model_params.set_parameter("model_type", get_model_type_by_name(model_name))
    model_params.set_parameter("epochs", epochs)
    model_params.set_parameter("ranking_size", ranking_size)
    model_params.set_parameter("rankings_per_image", rankings_per_image)
    model_params.set_parameter('val_rankings_per_img', rankings_per_image)
    model_params.set_parameter("batch_size", batch_size)
    model_params.set_parameter("seed", seed)
    model_params.set_parameter('equality_threshold', equality_threshold)
    model_params.set_parameter('loss_type', DepthLossType.NLL)
    model_params.set_parameter('augmentation', augmentation)
    model_params.set_parameter('warmup', warmup)
    if sampling_type == 0:
        sampling_strategy = ThresholdedMaskedRandomSamplingStrategy(model_params)
    elif sampling_type == 1:
        sampling_strategy = InformationScoreBasedSampling(model_params)
    elif sampling_type == 3:
        sampling_strategy = PurelyMaskedRandomSamplingStrategy(model_params)
    else:
        print("wrong sampling type")
        return 13
    model_params.set_parameter('sampling_strategy', sampling_strategy)
    model_input_shape = [224, 224, 3]
    model, preprocess_fn = get_pl_depth_net(model_params, model_input_shape)

    data = config["DATA"]
    if "HR_WSI_3K_PATH" in data:  # active_PLDepth.py:136-139
        from ..data.dao.hr_wsi import HRWSITFDataAccessObject
        dao = HRWSITFDataAccessObject(data["HR_WSI_3K_PATH"], model_input_shape, seed)
        imgs, gts, masks = dao.get_training_dataset(size=ds_size)
        val_imgs, val_gts, val_masks = dao.get_validation_dataset()
        gts, val_gts = gts[..., 0], val_gts[..., 0]
    else:
        n = ds_size or 8 * batch_size
        imgs, gts, masks = synthetic_hrwsi(n, 224, 224, seed)
        val_imgs, val_gts, val_masks = synthetic_hrwsi(max(batch_size, n // 15), 224, 224,
                                                       seed + 1)
    if "HR_WSI_POOL_PATH" in data:  # active_PLDepth.py:163-168
        from ..data.dao.hr_wsi import HRWSITFDataAccessObject
        dao_a = HRWSITFDataAccessObject(data["HR_WSI_POOL_PATH"], model_input_shape, seed=seed)
        pool_imgs, pool_gts, _ = dao_a.get_training_dataset(5000)
    else:
        pool_imgs, pool_gts, _ = synthetic_hrwsi(ds_size or 8 * batch_size, 224, 224, seed + 2)
    ds_size = len(imgs)

    steps_per_epoch = max(1, int((ds_size * 14 / 15) / batch_size))
    schedule = SGDRScheduler(min_lr=initial_lr * (1 / lr_multi), max_lr=initial_lr,
                             steps_per_epoch=steps_per_epoch, lr_decay=0.5,
                             cycle_length=epochs + 6, mult_factor=1)
    loss_fn = HourglassNegativeLogLikelihood(ranking_size=ranking_size, batch_size=batch_size)
    model.compile(loss=loss_fn, optimizer=Adam(learning_rate=initial_lr, amsgrad=True))
    if load_model_path:
        model.load_weights(load_model_path)
    data_provider = HourglassLargeScaleDataProvider(model_params, masks, val_masks,
                                                    augmentation=augmentation, seed=seed)
    train_ds = data_provider.provide_train_dataset(preprocess_fn(imgs), gts)
    val_ds = data_provider.provide_val_dataset(preprocess_fn(val_imgs), val_gts)
    callbacks = [TerminateOnNaN(), schedule, LearningRateLoggingCallback()]
    if model_checkpoints:
        from ..util.tracking_utils import construct_model_checkpoint_callback
        callbacks.append(construct_model_checkpoint_callback(config, model_name, 1))
    steps_per_epoch = max(1, int(ds_size / batch_size))  # active_PLDepth.py:156
    model.fit(x=train_ds, epochs=epochs, steps_per_epoch=steps_per_epoch, callbacks=callbacks,
              validation_data=val_ds, verbose=1)

    print("Start active sampling")
    run_active_rounds(model, pool_imgs, pool_gts, val_ds, batch_size=batch_size,
                      ranking_size=ranking_size, epochs=epochs, callbacks=callbacks,
                      schedule=schedule, img_size=model_input_shape)

    # evaluate on test data (active_PLDepth.py:191-198)
    err = calc_err(model, val_imgs[:300], val_gts[:300, ..., None],
                   img_size=tuple(model_input_shape[:2]))
    print(f"test_error {err:.6f}")
    return 0


if __name__ == "__main__":
    perform_pldepth_experiment()
