# builds the C++ mirror of the dense mesh (tests/test_tsdf_gpu.py) against the in-tree libsfmhip.so
tsdf_test: tsdf_test.cpp ../../sfm_opencv_amd/host/sfm_ops.hpp ../../include/sfmhip.h
	g++ -O2 -std=c++17 -Wall -o $@ tsdf_test.cpp -L../../sfm_opencv_amd -lsfmhip -Wl,-rpath,'$$ORIGIN/../../sfm_opencv_amd' -Wl,-rpath,/opt/rocm/lib
