#!/usr/bin/env python
"""Command-line entry with the reference's flags (main.py:9-28 / config/configurator.py:7-10):

    python main.py --model lightgcn [--dataset yelp|gowalla|amazon] [--device cuda] [--cuda 0]
                   [--synthetic amazon-book|yelp|gowalla|tiny]
    python main.py --model mhcn [--dataset ciao|epinions|yelp|lastfm] [--synthetic social-yelp|social-epinions|social-tiny]
    python main.py --model kgin [--dataset mind|alibaba-fashion|last-fm] [--synthetic kg-last-fm|kg-alibaba|kg-tiny]
    python main.py --model kgcl [--dataset mind|alibaba-fashion|last-fm] [--synthetic kg-last-fm|kg-alibaba|kg-tiny]
    python main.py --model kgrec [--dataset mind|alibaba-fashion|last-fm] [--synthetic kg-last-fm|kg-alibaba|kg-tiny]

Datasets are read from `./datasets/general_cf/sparse_*/{train,valid,test}_mat.pkl` (social models:
`./datasets/social/*/{trn,tst,trust}_mat.pkl`; kg models: `./datasets/kg/*_kg/{train,test,kg_final}.txt`)
relative to the working directory, exactly like
upstream; `--synthetic` (an addition) generates a seeded graph of a BASELINE shape instead, for
machines without the pickles."""
import sys


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    synthetic = None
    if '--synthetic' in argv:
        i = argv.index('--synthetic')
        synthetic = argv[i + 1]
        del argv[i:i + 2]
    from sslrec_amd.config.configurator import configs, parse_configure
    parse_configure(argv)
    if synthetic is not None:
        configs['data']['synthetic'] = synthetic
    if configs['tune']['enable']:
        raise NotImplementedError('grid search (tune.enable) is outside the scope of this implementation')
    from sslrec_amd.data_utils.build_data_handler import build_data_handler
    from sslrec_amd.models.bulid_model import build_model
    from sslrec_amd.trainer.build_trainer import build_trainer
    from sslrec_amd.trainer.logger import Logger
    from sslrec_amd.trainer.trainer import init_seed

    init_seed()
    data_handler = build_data_handler()
    data_handler.load_data()
    model = build_model(data_handler).to(configs['device'])
    logger = Logger()
    trainer = build_trainer(data_handler, logger)
    best_model = trainer.train(model)
    trainer.test(best_model)
    return best_model


if __name__ == '__main__':
    main()
