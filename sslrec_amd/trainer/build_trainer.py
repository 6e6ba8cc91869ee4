"""Trainer factory (reference trainer/build_trainer.py:4-13).  The reference picks a
model-specific trainer class when `configs['train']['trainer']` names one; AutoCF (`autocf_trainer`), AdaGCL (`AdaGCLTrainer`),
GFormer (`gformer_trainer`) and KGCL (`kgcl_trainer`) have their own, every other model of this path uses the generic `Trainer`.
`gformer_trainer` calls `preSelect_anchor_set`, `localGraph` and `masker`, which only GFormer has: it is built for model `gformer` and refused by name under
any other model.  `kgcl_trainer` calls `get_aug_views` once per epoch: it is refused by name for a model that has none."""
from ..config.configurator import configs
from .trainer import AdaGCLTrainer, AutoCFTrainer, GFormerTrainer, KGCLTrainer, Trainer


def build_trainer(data_handler, logger):
    name = configs['train'].get('trainer')
    if name is not None and name.lower() == 'autocf_trainer':
        return AutoCFTrainer(data_handler, logger)
    if name is not None and name.lower() == 'adagcltrainer':
        return AdaGCLTrainer(data_handler, logger)
    if name is not None and name.lower() == 'gformer_trainer':
        if str(configs['model'].get('name', '')).lower() != 'gformer':
            raise NotImplementedError('Trainer gformer_trainer is implemented for the model gformer only (it calls preSelect_anchor_set, '
                                      'localGraph and masker), not for {}'.format(configs['model'].get('name')))
        return GFormerTrainer(data_handler, logger)
    if name is not None and name.lower() == 'kgcl_trainer':
        if str(configs['model'].get('name', '')).lower() != 'kgcl':
            raise NotImplementedError('Trainer kgcl_trainer is implemented for the model kgcl only (it calls get_aug_views once per epoch), '
                                      'not for {}'.format(configs['model'].get('name')))
        return KGCLTrainer(data_handler, logger)
    if name is not None and name.lower() != 'trainer':
        raise NotImplementedError('Trainer {} is not implemented for the general-CF hot path'.format(name))
    return Trainer(data_handler, logger)
