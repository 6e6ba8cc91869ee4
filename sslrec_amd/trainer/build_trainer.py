"""Trainer factory (reference trainer/build_trainer.py:4-13).  The reference picks a
model-specific trainer class when `configs['train']['trainer']` names one; AutoCF (`autocf_trainer`) and AdaGCL (`AdaGCLTrainer`)
have their own, every other model of this path uses the generic `Trainer`."""
from ..config.configurator import configs
from .trainer import AdaGCLTrainer, AutoCFTrainer, Trainer


def build_trainer(data_handler, logger):
    name = configs['train'].get('trainer')
    if name is not None and name.lower() == 'autocf_trainer':
        return AutoCFTrainer(data_handler, logger)
    if name is not None and name.lower() == 'adagcltrainer':
        return AdaGCLTrainer(data_handler, logger)
    if name is not None and name.lower() != 'trainer':
        raise NotImplementedError('Trainer {} is not implemented for the general-CF hot path'.format(name))
    return Trainer(data_handler, logger)
