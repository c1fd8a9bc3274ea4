from .data_augmentor import DataAugmentor, DeviceDataAugmentor

__all__ = ['DataAugmentor', 'DeviceDataAugmentor']
