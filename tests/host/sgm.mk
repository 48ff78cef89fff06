# builds the C++ mirror of the dense step with the semi-global path on (tests/test_sgm_gpu.py) against the in-tree libsfmhip.so
sgm_test: sgm_test.cpp ../../sfm_opencv_amd/host/sfm_ops.hpp ../../include/sfmhip.h
	g++ -O2 -std=c++17 -Wall -o $@ sgm_test.cpp -L../../sfm_opencv_amd -lsfmhip -Wl,-rpath,'$$ORIGIN/../../sfm_opencv_amd' -Wl,-rpath,/opt/rocm/lib
